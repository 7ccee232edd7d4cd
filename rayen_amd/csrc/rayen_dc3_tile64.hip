// method='DC3' in fp64 on 16-sample tiles on the fp64 matrix cores: the twins of rayen_dc3_tile.hip's two kernels (same
// mathematics, same batch-global stop protocol, same contract; see that header and rayen_dc3.hip's) on
// v_mfma_f64_16x16x4_f64, for fp64 inputs on sets the fp64 lane kernel does not stage: 33 <= n <= 64, or an fp64 image over
// LDS.  The reference is trained in fp64 (header of rayen_mfma_f64.hip).
//
//     r = relu(A1e p - b1e),  g_i = 0.5 p'Pe_i p + qe_i'p + re_i,  u_i = Pe_i p + qe_i
//     grad = 2 A1e' r + sum_i 2 u_i relu(g_i),   s <- lr grad + momentum s,   p <- p - s
//     y[partial] = p,  y[other] = c0 + C p
//
// Layout (rayen_mfma_f64.hip's).  One workgroup of four waves owns a tile of 16 consecutive samples: a sample is a COLUMN
// of every product.  p, s and grad (n x 16, n <= 64: NX = 1 .. 4 blocks of 16 rows) live in MFMA accumulator layout, 4
// registers (doubles) a block, in EVERY wave (identical copies).  Lane l, register g of a block is column l & 15, row
// 4 g + (l >> 4); the B operand of a K-step is B[k = l >> 4][j = l & 15]: so register g of p IS the B operand of K-step g of
// its block of A1e p, with no permutation of k, and a block of relu'd residuals is the B operand of A1e_b' r_b.  The host
// stores the A images in per-lane order, two K-steps a 16-byte piece (rayen_dc3_tile64_image.h): one load feeds two MFMAs.
// The images are STREAMED from global memory (L2-resident); none is held in LDS.
//
// Nothing whose size depends on m, nq or no is held: a block of r is consumed by A1e_b' r_b as soon as it is produced; a
// u_i is folded into grad once its g_i is known (an in-lane sum over the lane's rows of p .* (u_i + qe_i), and two
// exchanges between the four lane groups that hold a column).  The work items -- the row blocks of A1e, then the
// quadratics -- go to the waves round robin; the four partial grads meet in LDS (two workgroup barriers a step; 8 KiB a
// block of n) and every wave then updates its copy of (p, s) identically.  The order of every sum is fixed by the set
// alone: a column's arithmetic does not depend on its tile-mates or on B (MFMA columns do not mix, the exchanges stay
// inside a column and add commutatively: all four lanes of a row group get the same bits).
//
// Stop protocol: rayen_dc3.hip's, unchanged -- launches of kChunk steps, viol[t] by atomic max on the 64 bits of a
// non-negative double (NaN as one canonical pattern; columns beyond B take no part), a launch leaves without writing if an
// earlier step met the rule, (p, s) ping-pong between two state buffers (in register order, [tile][2 NX][4][64]), one
// finishing launch that finds t*, replays t* - t0 steps where needed and writes t*.  The backward recomputes p_0 .. p_{T-1}
// into the workspace ([T][tile][NX][4][64]) and sweeps back with the J'x of rayen_dc3.hip's header; lr J' sbar is summed on
// its own and added to pbar once per step, as there.  lr, momentum and eps stay double.
// Envelope: rayen::dc3_tile64_served() (rayen_dc3_tile64_image.h) -- fp64, 1 <= n <= 64, the image within 1 GiB.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <vector>

#include "rayen_dc3_pack.h"
#include "rayen_dc3_tile64_image.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kTile = 16;                     // samples per workgroup
constexpr int kChunk = 32;                    // steps per launch (rayen_dc3.hip's)
constexpr unsigned long long kNanBits = 0x7ff8000000000000ull;

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

struct Img {
  const f64x2 *A, *AT, *P, *PT, *C, *CT;
  const double *b, *q, *r, *c0;
  int n, no, Mb, nq, Cb, kp;
};

Img img_of(const RayenDc3Pack* p) {
  const rayen::Dc3Tile64Dims d = rayen::dc3_tile64_dims(p->n, p->m, p->nq, p->no);
  const double* base = p->tile_img64;
  auto f2 = [&](int64_t off) { return reinterpret_cast<const f64x2*>(base + off); };
  Img im;
  im.A = f2(d.off_A); im.AT = f2(d.off_AT); im.P = f2(d.off_P); im.PT = f2(d.off_PT); im.C = f2(d.off_C); im.CT = f2(d.off_CT);
  im.b = base + d.off_b; im.q = base + d.off_q; im.r = base + d.off_r; im.c0 = base + d.off_c0;
  im.n = d.n; im.no = d.no; im.Mb = d.Mb; im.nq = d.nq; im.Cb = d.Cb; im.kp = d.kp;
  return im;
}

__device__ __forceinline__ int row_of(int g, int grp) { return 4 * g + grp; }

__device__ __forceinline__ double bits_to_double(unsigned long long b) { return __longlong_as_double((long long)b); }

// max that keeps a NaN once it has seen one (torch.max over a batch with a NaN is NaN)
__device__ __forceinline__ double max_nan(double acc, double x) { return (x > acc || x != x) ? x : acc; }

__device__ __forceinline__ void record_violation(unsigned long long* slot, double v, bool live) {
  if (!live) v = 0.0;
  for (int off = 32; off > 0; off >>= 1) v = max_nan(v, __shfl_xor(v, off, 64));
  if ((threadIdx.x & 63) == 0) {
    const unsigned long long bits = v != v ? kNanBits : (unsigned long long)__double_as_longlong(v);
    if (bits != 0) atomicMax(slot, bits);
  }
}

#define RAYEN_MFMA2(A, SRC, BASE, ACC)                                                  \
  ACC = __builtin_amdgcn_mfma_f64_16x16x4f64((A).x, (SRC)[(BASE) + 0], ACC, 0, 0, 0);   \
  ACC = __builtin_amdgcn_mfma_f64_16x16x4f64((A).y, (SRC)[(BASE) + 1], ACC, 0, 0, 0)

// a block of 16 values in accumulator layout from a plain array of whole blocks (b1e, qe_i, c0)
__device__ __forceinline__ f64x4 load_block(const double* __restrict__ v, int grp) {
  f64x4 acc;
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = v[4 * g + grp];
  return acc;
}

// acc += M_block src, M_block a rows-image block ([kp][64] pairs at `Mb`)
template <int NX>
__device__ __forceinline__ void times_rows(const f64x2* __restrict__ Mb, int kp, int lane, const f64x4 (&src)[NX],
                                           f64x4& acc) {
#pragma unroll
  for (int gp = 0; gp < 2 * NX; ++gp)
    if (gp < kp) {
      const f64x2 A = Mb[gp * 64 + lane];
      RAYEN_MFMA2(A, src[gp >> 1], 2 * (gp & 1), acc);
    }
}

// out += M_block' src, M_block a columns-image block ([NX][2][64] pairs at `Mb`), src one block of 16 rows
template <int NX>
__device__ __forceinline__ void times_columns(const f64x2* __restrict__ Mb, int lane, const f64x4& src, f64x4 (&out)[NX]) {
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      const f64x2 A = Mb[(ob * 2 + gp) * 64 + lane];
      RAYEN_MFMA2(A, src, 2 * gp, out[ob]);
    }
}

template <int NX>
__device__ __forceinline__ void zero(f64x4 (&x)[NX]) {
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < 4; ++i) x[ob][i] = 0.0;
}

// the sum over a column of a value each lane holds for its rows: the four lane groups of a column exchange twice (the
// additions commute: every lane of the column ends with the same bits)
__device__ __forceinline__ double column_sum(double v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// the first quadratic of `wave`: the work items (row blocks, then quadratics) go round robin
__device__ __forceinline__ int first_quadratic(const Img& im, int wave) { return (wave + kWaves - im.Mb % kWaves) % kWaves; }

// u = Pe_c p + qe_c, qv = qe_c; returns g_c (the same in the four lanes of a column)
template <int NX>
__device__ __forceinline__ double quadratic(const Img& im, int c, int lane, const f64x4 (&p)[NX], f64x4 (&u)[NX],
                                            f64x4 (&qv)[NX]) {
  const int grp = lane >> 4;
#pragma unroll
  for (int ob = 0; ob < NX; ++ob) {
    qv[ob] = load_block(im.q + ((size_t)c * NX + ob) * 16, grp);
    u[ob] = qv[ob];
    times_rows<NX>(im.P + ((size_t)c * NX + ob) * im.kp * 64, im.kp, lane, p, u[ob]);
  }
  double g2 = 0.0;
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < 4; ++i) g2 = fma(p[ob][i], u[ob][i] + qv[ob][i], g2);
  return fma(0.5, column_sum(g2), im.r[c]);
}

// This wave's share of the residuals at p: returns max(0, its linear residuals, its g_i) (NaN kept); with GRAD also its
// share of the correction direction, added to `part`.
template <int NX, bool GRAD>
__device__ __forceinline__ double eval_share(const Img& im, int wave, int lane, const f64x4 (&p)[NX], f64x4 (&part)[NX]) {
  const int grp = lane >> 4;
  double viol = 0.0;
  for (int b = wave; b < im.Mb; b += kWaves) {
    f64x4 acc = load_block(im.b + (size_t)b * 16, grp);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = -acc[i];
    times_rows<NX>(im.A + (size_t)b * im.kp * 64, im.kp, lane, p, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double r = acc[i];
      viol = max_nan(viol, r);
      acc[i] = r > 0.0 ? r + r : (r != r ? r : 0.0);
    }
    if constexpr (GRAD) times_columns<NX>(im.AT + (size_t)b * NX * 128, lane, acc, part);
  }
  for (int c = first_quadratic(im, wave); c < im.nq; c += kWaves) {
    f64x4 u[NX], qv[NX];
    const double g = quadratic<NX>(im, c, lane, p, u, qv);
    viol = max_nan(viol, g);
    if constexpr (GRAD) {
      const double gg = g > 0.0 ? g + g : (g != g ? g : 0.0);
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < 4; ++i) part[ob][i] = fma(u[ob][i], gg, part[ob][i]);
    }
  }
  return viol;
}

// part += this wave's share of lr J(p)' x   (J of the correction direction at p; rayen_dc3.hip's header)
template <int NX>
__device__ __forceinline__ void jacobian_transpose_share(const Img& im, int wave, int lane, const f64x4 (&p)[NX],
                                                         const f64x4 (&x)[NX], double lr, f64x4 (&part)[NX]) {
  const int grp = lane >> 4;
  const double lr2 = lr + lr;
  for (int b = wave; b < im.Mb; b += kWaves) {
    f64x4 r = load_block(im.b + (size_t)b * 16, grp), dx;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      r[i] = -r[i];
      dx[i] = 0.0;
    }
    const f64x2* __restrict__ Ab = im.A + (size_t)b * im.kp * 64;
#pragma unroll
    for (int gp = 0; gp < 2 * NX; ++gp)
      if (gp < im.kp) {
        const f64x2 A = Ab[gp * 64 + lane];
        RAYEN_MFMA2(A, p[gp >> 1], 2 * (gp & 1), r);
        RAYEN_MFMA2(A, x[gp >> 1], 2 * (gp & 1), dx);
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) dx[i] = r[i] > 0.0 ? lr2 * dx[i] : 0.0;
    times_columns<NX>(im.AT + (size_t)b * NX * 128, lane, dx, part);
  }
  for (int c = first_quadratic(im, wave); c < im.nq; c += kWaves) {
    f64x4 u[NX], qv[NX];
    const double g = quadratic<NX>(im, c, lane, p, u, qv);
    double w = 0.0;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) w = fma(u[ob][i], x[ob][i], w);
    w = column_sum(w);
    if (__any(g > 0.0)) {
      // 2 (relu(g) Pe' x + [g > 0] w (0.5 (Pe + Pe') p + qe)) = Pe' (2 relu(g) x + [g > 0] w p) + [g > 0] w (u + qe)
      const double cg = g > 0.0 ? lr2 * g : 0.0;
      const double cw = g > 0.0 ? lr * w : 0.0;
      f64x4 z[NX];
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < 4; ++i) z[ob][i] = fma(cg, x[ob][i], cw * p[ob][i]);
#pragma unroll
      for (int ob = 0; ob < NX; ++ob) {
        times_rows<NX>(im.PT + ((size_t)c * NX + ob) * im.kp * 64, im.kp, lane, z, part[ob]);
#pragma unroll
        for (int i = 0; i < 4; ++i) part[ob][i] = fma(cw, u[ob][i] + qv[ob][i], part[ob][i]);
      }
    }
  }
}

// The four waves' partial sums meet in LDS; every wave leaves with the same total.  Two workgroup barriers.
template <int NX>
__device__ __forceinline__ void sum_partials(double* Pbuf, int wave, int lane, const f64x4 (&part)[NX], f64x4 (&total)[NX]) {
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < 4; ++i) Pbuf[((wave * NX + ob) * 4 + i) * 64 + lane] = part[ob][i];
  __syncthreads();
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int at = (ob * 4 + i) * 64 + lane;
      total[ob][i] = (Pbuf[at] + Pbuf[NX * 256 + at]) + (Pbuf[2 * NX * 256 + at] + Pbuf[3 * NX * 256 + at]);
    }
  __syncthreads();
}

// one step from (p, s): every wave ends with the same new (p, s); returns this wave's share of the violation AT the old p
template <int NX>
__device__ __forceinline__ double step(const Img& im, double* Pbuf, int wave, int lane, double lr, double momentum,
                                       f64x4 (&p)[NX], f64x4 (&s)[NX]) {
  f64x4 part[NX], grad[NX];
  zero<NX>(part);
  const double v = eval_share<NX, true>(im, wave, lane, p, part);
  sum_partials<NX>(Pbuf, wave, lane, part, grad);
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s[ob][i] = lr * grad[ob][i] + momentum * s[ob][i];
      p[ob][i] -= s[ob][i];
    }
  return v;
}

// rows of the caller's arrays <-> accumulator layout (columns beyond B: zero in, nothing out)
template <int NX>
__device__ __forceinline__ void load_rows(const double* __restrict__ row, bool live, int n, int grp, f64x4 (&x)[NX]) {
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 16 * ob + row_of(i, grp);
      x[ob][i] = (live && j < n) ? row[j] : 0.0;
    }
}

template <int NX>
__device__ __forceinline__ void load_state(const double* __restrict__ src, bool live, int lane, f64x4 (&x)[NX]) {
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < 4; ++i) x[ob][i] = live ? src[(ob * 4 + i) * 64 + lane] : 0.0;
}

template <int NX>
__device__ __forceinline__ void store_state(double* __restrict__ dst, bool live, int lane, const f64x4 (&x)[NX]) {
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (live) dst[(ob * 4 + i) * 64 + lane] = x[ob][i];
}

struct FwdArgs {
  Img im;
  const int32_t* perm;
  const double* q;
  int64_t B, ldq;
  double* y;
  int64_t ldy;
  double lr, momentum, eps;
  int max_steps;
  int chunk;                 // >= 0: run chunk `chunk`; -1: the finishing launch
  unsigned long long* viol;  // [max_steps + 1]
  double* state0;            // [tiles][2 NX][4][64] each: p then s (nullptr with a single chunk)
  double* state1;
  int32_t* tstar;
  int32_t* nan_flag;
};

template <int NX>
__global__ __launch_bounds__(kThreads) void dc3_tile64_forward_kernel(const FwdArgs a) {
  __shared__ double Pbuf[kWaves * NX * 256];
  __shared__ int sh_t;
  const Img& im = a.im;
  int chunk = a.chunk, nsteps;
  const bool record = chunk >= 0;
  if (record) {
    const int t0 = chunk * kChunk;
    if (threadIdx.x == 0) sh_t = 0;
    __syncthreads();
    for (int t = 1 + (int)threadIdx.x; t <= t0; t += kThreads)
      if (bits_to_double(a.viol[t]) < a.eps) atomicOr(&sh_t, 1);
    __syncthreads();
    if (sh_t) return;                             // an earlier step already met the stop rule: write nothing
    nsteps = a.max_steps - t0 < kChunk ? a.max_steps - t0 : kChunk;
  } else {
    if (threadIdx.x == 0) sh_t = a.max_steps;
    __syncthreads();
    for (int t = 1 + (int)threadIdx.x; t < a.max_steps; t += kThreads)
      if (bits_to_double(a.viol[t]) < a.eps) atomicMin(&sh_t, t);
    __syncthreads();
    const int ts = sh_t;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.tstar = ts;
    chunk = (ts - 1) / kChunk;
    const int t0 = chunk * kChunk;
    const int end = a.max_steps - t0 < kChunk ? a.max_steps : t0 + kChunk;
    if (ts == end) return;                        // that chunk's own y is the answer
    nsteps = ts - t0;
  }
  const int lane = threadIdx.x & 63, grp = lane >> 4, col = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);        // (uniform, and the compiler knows it)
  const int64_t tile = blockIdx.x;
  const int64_t sample = tile * kTile + col;
  const bool live = sample < a.B;
  const int n = im.n;
  f64x4 p[NX], s[NX];
  if (chunk == 0) {
    load_rows<NX>(a.q + (live ? sample : 0) * a.ldq, live, n, grp, p);
    zero<NX>(s);
  } else {
    const double* src = ((chunk & 1) ? a.state1 : a.state0) + (size_t)tile * 2 * NX * 256;
    load_state<NX>(src, live, lane, p);
    load_state<NX>(src + NX * 256, live, lane, s);
  }
  const int t0 = chunk * kChunk;
  for (int st = 0; st < nsteps; ++st) {
    const double v = step<NX>(im, Pbuf, wave, lane, a.lr, a.momentum, p, s);
    if (record && st >= 1) record_violation(a.viol + t0 + st, v, live);
  }
  if (record) {
    f64x4 none[NX];
    const double v = eval_share<NX, false>(im, wave, lane, p, none);
    record_violation(a.viol + t0 + nsteps, v, live);
    if (wave == 0 && t0 + nsteps < a.max_steps) {
      double* dst = ((chunk & 1) ? a.state0 : a.state1) + (size_t)tile * 2 * NX * 256;
      store_state<NX>(dst, live, lane, p);
      store_state<NX>(dst + NX * 256, live, lane, s);
    }
  }
  // y[partial] = p (wave 0), y[other] = c0 + C p (the row blocks of C round robin)
  double* __restrict__ yr = a.y + (live ? sample : 0) * a.ldy;
  bool bad = false;
  if (wave == 0) {
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 16 * ob + row_of(i, grp);
        if (live && j < n) {
          yr[a.perm[j]] = p[ob][i];
          bad |= p[ob][i] != p[ob][i];
        }
      }
  }
  for (int cb = wave; cb < im.Cb; cb += kWaves) {
    f64x4 acc = load_block(im.c0 + (size_t)cb * 16, grp);
    times_rows<NX>(im.C + (size_t)cb * im.kp * 64, im.kp, lane, p, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = 16 * cb + row_of(i, grp);
      if (live && o < im.no) {
        yr[a.perm[n + o]] = acc[i];
        bad |= acc[i] != acc[i];
      }
    }
  }
  if (bad && a.nan_flag != nullptr) atomicOr(a.nan_flag, 1);
}

struct BwdArgs {
  Img im;
  const int32_t* perm;
  const double* q;
  int64_t B, ldq;
  const double* grad_y;
  int64_t ldg;
  double* grad_q;
  int64_t ldgq;
  double lr, momentum;
  int max_steps;
  const int32_t* tstar;
  double* traj;              // [max_steps][tiles][NX][4][64]
};

template <int NX>
__global__ __launch_bounds__(kThreads) void dc3_tile64_backward_kernel(const BwdArgs a) {
  __shared__ double Pbuf[kWaves * NX * 256];
  const Img& im = a.im;
  const int lane = threadIdx.x & 63, grp = lane >> 4, col = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tile = blockIdx.x;
  const int64_t sample = tile * kTile + col;
  const bool live = sample < a.B;
  const int n = im.n;
  int T_steps = *a.tstar;
  if (T_steps > a.max_steps) T_steps = a.max_steps;
  const size_t tiles = gridDim.x;
  double* traj = a.traj + (size_t)tile * NX * 256;             // step t: + t * tiles * NX * 256
  const size_t tstride = tiles * NX * 256;
  f64x4 p[NX], s[NX], w[NX];
  load_rows<NX>(a.q + (live ? sample : 0) * a.ldq, live, n, grp, p);
  zero<NX>(s);
  for (int t = 0; t < T_steps; ++t) {
    if (wave == 0) store_state<NX>(traj + (size_t)t * tstride, live, lane, p);
    if (t + 1 < T_steps) (void)step<NX>(im, Pbuf, wave, lane, a.lr, a.momentum, p, s);
  }
  __syncthreads();           // wave 0's trajectory is read by every wave below
  // pbar_T = grad_y[partial] + C' grad_y[other]; s now holds sbar (zero beyond the last step)
  const double* __restrict__ gy = a.grad_y + (live ? sample : 0) * a.ldg;
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 16 * ob + row_of(i, grp);
      w[ob][i] = (live && j < n) ? gy[a.perm[j]] : 0.0;
    }
  f64x4 part[NX], dj[NX];
  if (im.Cb > 0) {
    zero<NX>(part);
    for (int cb = wave; cb < im.Cb; cb += kWaves) {
      f64x4 go;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = 16 * cb + row_of(i, grp);
        go[i] = (live && o < im.no) ? gy[a.perm[n + o]] : 0.0;
      }
      times_columns<NX>(im.CT + (size_t)cb * NX * 128, lane, go, part);
    }
    sum_partials<NX>(Pbuf, wave, lane, part, dj);
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) w[ob][i] += dj[ob][i];
  }
  zero<NX>(s);
  for (int t = T_steps - 1; t >= 0; --t) {
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) s[ob][i] = a.momentum * s[ob][i] - w[ob][i];
    load_state<NX>(traj + (size_t)t * tstride, live, lane, p);
    zero<NX>(part);
    jacobian_transpose_share<NX>(im, wave, lane, p, s, a.lr, part);
    sum_partials<NX>(Pbuf, wave, lane, part, dj);
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) w[ob][i] += dj[ob][i];
  }
  if (wave == 0) {
    double* __restrict__ gq = a.grad_q + (live ? sample : 0) * a.ldgq;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 16 * ob + row_of(i, grp);
        if (live && j < n) gq[j] = w[ob][i];
      }
  }
}

int n_chunks(int max_steps) { return (max_steps + kChunk - 1) / kChunk; }
size_t n_tiles(int64_t B) { return (size_t)((B + kTile - 1) / kTile); }
size_t n_blocks(const RayenDc3Pack* p) { return (size_t)(p->n + 15) / 16; }

// the scratch buffers: viol [max_steps + 1] | with more than one launch of steps, (p, s) in register order twice
enum { kViol = 0, kState0 = 1, kState1 = 2 };
rayen::WsLayout<3> forward_ws(const RayenDc3Pack* p, int64_t B, int max_steps) {
  const size_t state = n_chunks(max_steps) > 1 ? n_tiles(B) * 2 * n_blocks(p) * 256 : 0;
  return rayen::ws_layout<3>(
      {{sizeof(unsigned long long), (size_t)max_steps + 1}, {sizeof(double), state}, {sizeof(double), state}});
}

// the recomputed trajectory [max_steps][tiles][nx][4][64]
rayen::WsLayout<1> backward_ws(const RayenDc3Pack* p, int64_t B, int max_steps) {
  return rayen::ws_layout<1>({{sizeof(double), (size_t)max_steps * n_tiles(B) * n_blocks(p) * 256}});
}

bool served(const RayenDc3Pack* p) {
  return p != nullptr && p->tile_img64 != nullptr && p->perm != nullptr &&
         rayen::dc3_tile64_served(p->n, p->m, p->nq, p->no);
}

template <int NX>
int launch_forward(FwdArgs a, hipStream_t stream) {
  const unsigned grid = (unsigned)n_tiles(a.B);
  const int chunks = n_chunks(a.max_steps);
  for (int c = 0; c <= chunks; ++c) {
    a.chunk = c < chunks ? c : -1;
    hipLaunchKernelGGL(dc3_tile64_forward_kernel<NX>, dim3(grid), dim3(kThreads), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return RAYEN_E_LAUNCH;
  }
  return RAYEN_OK;
}

template <int NX>
int launch_backward(const BwdArgs& a, hipStream_t stream) {
  const unsigned grid = (unsigned)n_tiles(a.B);
  hipLaunchKernelGGL(dc3_tile64_backward_kernel<NX>, dim3(grid), dim3(kThreads), 0, stream, a);
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

}  // namespace

extern "C" {

int rayen_dc3_tile64_shape_served(int32_t n, int32_t m, int32_t nq, int32_t no) {
  return rayen::dc3_tile64_served(n, m, nq, no) ? 1 : 0;
}

int rayen_dc3_tile64_pack_set(RayenDc3Pack* p, const double* A1e, const double* b1e, const double* Pe, const double* qe,
                              const double* re, const double* C, const double* c0) {
  if (p == nullptr || (p->m > 0 && (A1e == nullptr || b1e == nullptr)) ||
      (p->nq > 0 && (Pe == nullptr || qe == nullptr || re == nullptr)) || (p->no > 0 && (C == nullptr || c0 == nullptr)))
    return RAYEN_E_BAD_ARG;
  if (p->tile_img64 != nullptr) return RAYEN_OK;
  std::vector<double> h;
  // a shape outside the envelope gets no image: the calls answer RAYEN_E_UNSUPPORTED
  if (!rayen::dc3_tile64_image(p->n, p->m, p->nq, p->no, A1e, b1e, Pe, qe, re, C, c0, &h)) return RAYEN_OK;
  const int rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK) return rc;
  if (!rayen::upload_image(h, &p->tile_img64)) {
    if (p->tile_img64) (void)hipFree(p->tile_img64);
    p->tile_img64 = nullptr;
    return RAYEN_E_ALLOC;
  }
  return RAYEN_OK;
}

int rayen_dc3_tile64_served(const RayenDc3Pack* pack) { return served(pack) ? 1 : 0; }

int64_t rayen_dc3_tile64_workspace_bytes(const RayenDc3Pack* p, int64_t B, int32_t max_steps, int32_t backward) {
  if (p == nullptr || B < 0 || max_steps < 1) return -1;
  return (int64_t)(backward ? backward_ws(p, B, max_steps).total : forward_ws(p, B, max_steps).total);
}

int rayen_dc3_tile64_forward_f64(const RayenDc3Pack* p, const double* q, int64_t B, int64_t ldq, double* y, int64_t ldy,
                                 double lr, double momentum, double eps, int32_t max_steps, int32_t* tstar, void* ws,
                                 int64_t ws_bytes, int32_t* nan_flag, void* stream) {
  if (p == nullptr || B < 0 || max_steps < 1 || tstar == nullptr) return RAYEN_E_BAD_ARG;
  if (B > 0 && (q == nullptr || y == nullptr || ldq < p->n || ldy < p->k)) return RAYEN_E_BAD_ARG;
  if (B > ((int64_t)1 << 31) - kThreads) return RAYEN_E_BAD_ARG;
  if (!served(p)) return RAYEN_E_UNSUPPORTED;
  const rayen::WsLayout<3> w = forward_ws(p, B, max_steps);
  if (ws == nullptr || ws_bytes < (int64_t)w.total) return RAYEN_E_BAD_ARG;
  const int rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(ws, 0, w.bytes[kViol], s) != hipSuccess) return RAYEN_E_LAUNCH;
  if (B == 0) {
    // an empty batch takes no step (the reference's maximum over nothing raises)
    return hipMemsetAsync(tstar, 0, sizeof(int32_t), s) == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
  }
  FwdArgs a;
  a.im = img_of(p);
  a.perm = p->perm;
  a.q = q; a.B = B; a.ldq = ldq; a.y = y; a.ldy = ldy;
  a.lr = lr; a.momentum = momentum; a.eps = eps;
  a.max_steps = max_steps;
  a.chunk = 0;
  a.viol = w.at<unsigned long long>(ws, kViol);
  a.state0 = w.at<double>(ws, kState0);      // (null with a single chunk)
  a.state1 = w.at<double>(ws, kState1);
  a.tstar = tstar;
  a.nan_flag = nan_flag;
  switch (n_blocks(p)) {
    case 1: return launch_forward<1>(a, s);
    case 2: return launch_forward<2>(a, s);
    case 3: return launch_forward<3>(a, s);
    default: return launch_forward<4>(a, s);
  }
}

int rayen_dc3_tile64_backward_f64(const RayenDc3Pack* p, const double* q, int64_t B, int64_t ldq, const double* grad_y,
                                  int64_t ldg, double* grad_q, int64_t ldgq, double lr, double momentum, int32_t max_steps,
                                  const int32_t* tstar, void* ws, int64_t ws_bytes, void* stream) {
  if (p == nullptr || B < 0 || max_steps < 1 || tstar == nullptr) return RAYEN_E_BAD_ARG;
  if (B > 0 && (q == nullptr || grad_y == nullptr || grad_q == nullptr || ldq < p->n || ldg < p->k || ldgq < p->n))
    return RAYEN_E_BAD_ARG;
  if (B > ((int64_t)1 << 31) - kThreads) return RAYEN_E_BAD_ARG;
  if (!served(p)) return RAYEN_E_UNSUPPORTED;
  const rayen::WsLayout<1> w = backward_ws(p, B, max_steps);
  if (B > 0 && (ws == nullptr || ws_bytes < (int64_t)w.total)) return RAYEN_E_BAD_ARG;
  const int rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK || B == 0) return rc;
  BwdArgs a;
  a.im = img_of(p);
  a.perm = p->perm;
  a.q = q; a.B = B; a.ldq = ldq; a.grad_y = grad_y; a.ldg = ldg; a.grad_q = grad_q; a.ldgq = ldgq;
  a.lr = lr; a.momentum = momentum;
  a.max_steps = max_steps;
  a.tstar = tstar;
  a.traj = w.at<double>(ws, 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (n_blocks(p)) {
    case 1: return launch_backward<1>(a, s);
    case 2: return launch_backward<2>(a, s);
    case 3: return launch_backward<3>(a, s);
    default: return launch_backward<4>(a, s);
  }
}

}  // extern "C"
