// method='DC3' on sample tiles on the matrix cores, once for both precisions: the iteration of rayen_dc3.hip (same
// mathematics, same batch-global stop protocol, same contract; see that header) for sets whose image does not fit LDS.
// rayen_dc3_tile.hip instantiates it for fp32 (Dc3Geom32), rayen_dc3_tile64.hip for fp64 (Dc3Geom64); each MFMA is bit for
// bit an fma chain: the differences from the lane kernels are summation order.
//
//     r = relu(A1e p - b1e),  g_i = 0.5 p'Pe_i p + qe_i'p + re_i,  u_i = Pe_i p + qe_i
//     grad = 2 A1e' r + sum_i 2 u_i relu(g_i),   s <- lr grad + momentum s,   p <- p - s
//     y[partial] = p,  y[other] = c0 + C p
//
// The two geometries (R = rows of a block = samples of a tile; everything else follows from R and the pack):
//                               Dc3Geom32                          Dc3Geom64
//     MFMA                      v_mfma_f32_32x32x2_f32             v_mfma_f64_16x16x4_f64
//     R                         32                                 16
//     blocks of n (NX)          1 .. 2                             1 .. 4
//     registers a block R^2/64  16                                 4
//     lane groups 64/R          2 (half-waves)                     4
//     operand pack              float4: four K-steps               two doubles: two K-steps
//     row of register i         8 (i >> 2) + 4 grp + (i & 3)       4 i + grp
//     violation slot            32 bits                            64 bits
//
// Layout.  One workgroup of four waves owns a tile of R consecutive samples: a sample is a COLUMN of every product.  p, s
// and grad (n x R, n <= 64: NX blocks of R rows) live in MFMA accumulator layout in EVERY wave (identical copies).  Lane l,
// register i of a block is column l % R, row row_of(i, l / R); the B operand of a K-step is B[k = l / R][j = l % R]: so
// register i of p IS the B operand of one K-step of A1e p, and a block of relu'd residuals is the B operand of A1e_b' r_b.
// The host stores the A images with k ordered to match and in per-lane order (rayen_dc3_tile_image.h): one coalesced
// 16-byte load a lane feeds a pack's MFMAs.  The images are STREAMED from global memory (L2-resident); none is held in LDS.
//
// Nothing whose size depends on m, nq or no is held: a block of r is consumed by A1e_b' r_b as soon as it is produced; a
// u_i is folded into grad once its g_i is known (an in-lane sum over the lane's rows of p .* (u_i + qe_i), and the exchanges
// between the lane groups that hold a column).  The work items -- the row blocks of A1e, then the quadratics -- go to the
// waves round robin; the four partial grads meet in LDS (two workgroup barriers a step) and every wave then updates its
// copy of (p, s) identically.  The order of every sum is fixed by the set alone: a column's arithmetic does not depend on
// its tile-mates or on B (MFMA columns do not mix, the exchanges stay inside a column and add commutatively: all lanes of
// a column get the same bits).
//
// Stop protocol: rayen_dc3.hip's, unchanged -- launches of kChunk steps, viol[t] by atomic max on the bits of a
// non-negative value (NaN as one canonical pattern; columns beyond B take no part), a launch leaves without writing if an
// earlier step met the rule, (p, s) ping-pong between two state buffers (in register order, [tile][2 NX][regs][64]), one
// finishing launch that finds t*, replays t* - t0 steps where needed and writes t*.  The backward recomputes
// p_0 .. p_{T-1} into the workspace ([T][tile][NX][regs][64]) and sweeps back with the J'x of rayen_dc3.hip's header;
// lr J' sbar is summed on its own and added to pbar once per step, as there.  lr, momentum and eps are rounded to the
// kernel's precision.  Envelope: Layout::served() (rayen_dc3_tile_image.h) -- 1 <= n <= 64, the image within 1 GiB.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <type_traits>
#include <vector>

#include "rayen_dc3_pack.h"
#include "rayen_dc3_tile_image.h"

namespace rayen {
namespace dc3_tile {

// ---------------------------------------------------------------------------------------------------- the two geometries
// What a geometry states: the scalar, block and pack types, the image layout (rows of a block, elements of a pack, row_of),
// the MFMAs of one pack, the violation word, the most blocks of n, the pack's image field -- and load_block, which fp32
// reads as float4 (the compiler does not merge the four loads of a register group on its own).

struct Dc3Geom32 {
  using T = float;
  using Layout = Dc3TileLayout32;
  typedef float Block __attribute__((ext_vector_type(16)));
  using Pack = float4;
  using Word = unsigned int;
  static constexpr Word kNanBits = 0x7fc00000u;
  static constexpr int kMaxNX = 2;
  static constexpr float* RayenDc3Pack::*kImage = &RayenDc3Pack::tile_img;
  static __device__ __forceinline__ Word to_bits(float v) { return __float_as_uint(v); }
  static __device__ __forceinline__ float from_bits(Word b) { return __uint_as_float(b); }
  // acc += the four K-steps of pack A against registers base .. base + 3 of src
  static __device__ __forceinline__ void mfma_pack(const Pack& A, const Block& src, const int base, Block& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A.x, src[base + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A.y, src[base + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A.z, src[base + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A.w, src[base + 3], acc, 0, 0, 0);
  }
  // a block of 32 values in accumulator layout from a plain array of whole blocks (b1e, qe_i, c0)
  static __device__ __forceinline__ Block load_block(const float* __restrict__ v, const int half) {
    const float4* v4 = reinterpret_cast<const float4*>(v);
    Block acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 x = v4[2 * g + half];
      acc[4 * g + 0] = x.x; acc[4 * g + 1] = x.y; acc[4 * g + 2] = x.z; acc[4 * g + 3] = x.w;
    }
    return acc;
  }
};

struct Dc3Geom64 {
  using T = double;
  using Layout = Dc3TileLayout64;
  typedef double Block __attribute__((ext_vector_type(4)));
  typedef double Pack __attribute__((ext_vector_type(2)));
  using Word = unsigned long long;
  static constexpr Word kNanBits = 0x7ff8000000000000ull;
  static constexpr int kMaxNX = 4;
  static constexpr double* RayenDc3Pack::*kImage = &RayenDc3Pack::tile_img64;
  static __device__ __forceinline__ Word to_bits(double v) { return (Word)__double_as_longlong(v); }
  static __device__ __forceinline__ double from_bits(Word b) { return __longlong_as_double((long long)b); }
  // acc += the two K-steps of pack A against registers base, base + 1 of src
  static __device__ __forceinline__ void mfma_pack(const Pack& A, const Block& src, const int base, Block& acc) {
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A.x, src[base + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A.y, src[base + 1], acc, 0, 0, 0);
  }
  // a block of 16 values in accumulator layout from a plain array of whole blocks (b1e, qe_i, c0)
  static __device__ __forceinline__ Block load_block(const double* __restrict__ v, const int grp) {
    Block acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = v[Layout::row_of(g, grp)];
    return acc;
  }
};

// ------------------------------------------------------------------------------------------- what follows from a geometry

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kChunk = 32;                    // steps per launch (rayen_dc3.hip's)

template <typename G> constexpr int kRows = G::Layout::kRows;                  // rows of a block = samples of a tile
template <typename G> constexpr int kRegs = kRows<G> * kRows<G> / 64;          // registers a block
template <typename G> constexpr int kPacks = kRegs<G> / G::Layout::kPack;      // packs a block
template <typename G> constexpr int kBlock = kRegs<G> * 64;                    // a block in register order (Pbuf, the states)

template <typename G> using Scalar = typename G::T;
template <typename G> using Block = typename G::Block;
template <typename G> using Pack = typename G::Pack;

template <typename G>
struct Img {
  const Pack<G> *A, *AT, *P, *PT, *C, *CT;
  const Scalar<G> *b, *q, *r, *c0;
  int n, no, Mb, nq, Cb, kp;
};

template <typename G>
Img<G> img_of(const RayenDc3Pack* p) {
  static_assert(sizeof(Block<G>) == kRegs<G> * sizeof(Scalar<G>) && sizeof(Pack<G>) == G::Layout::kPack * sizeof(Scalar<G>),
                "the block and the pack are what the layout says");
  const Dc3TileDims d = G::Layout::dims(p->n, p->m, p->nq, p->no);
  const Scalar<G>* base = p->*G::kImage;
  auto packs = [&](int64_t off) { return reinterpret_cast<const Pack<G>*>(base + off); };
  Img<G> im;
  im.A = packs(d.off_A); im.AT = packs(d.off_AT); im.P = packs(d.off_P); im.PT = packs(d.off_PT); im.C = packs(d.off_C);
  im.CT = packs(d.off_CT);
  im.b = base + d.off_b; im.q = base + d.off_q; im.r = base + d.off_r; im.c0 = base + d.off_c0;
  im.n = d.n; im.no = d.no; im.Mb = d.Mb; im.nq = d.nq; im.Cb = d.Cb; im.kp = d.kp;
  return im;
}

template <typename G>
__device__ __forceinline__ int row_of(int i, int grp) { return G::Layout::row_of(i, grp); }

// max that keeps a NaN once it has seen one (torch.max over a batch with a NaN is NaN)
template <typename T>
__device__ __forceinline__ T max_nan(T acc, T x) { return (x > acc || x != x) ? x : acc; }

template <typename G>
__device__ __forceinline__ void record_violation(typename G::Word* slot, Scalar<G> v, bool live) {
  if (!live) v = 0;
  for (int off = 32; off > 0; off >>= 1) v = max_nan(v, __shfl_xor(v, off, 64));
  if ((threadIdx.x & 63) == 0) {
    const typename G::Word bits = v != v ? G::kNanBits : G::to_bits(v);
    if (bits != 0) atomicMax(slot, bits);
  }
}

// acc += M_block src, M_block a rows-image block ([kp][64] packs at `Mb`)
template <typename G, int NX>
__device__ __forceinline__ void times_rows(const Pack<G>* __restrict__ Mb, int kp, int lane, const Block<G> (&src)[NX],
                                           Block<G>& acc) {
  constexpr int PB = kPacks<G>, PE = G::Layout::kPack;
#pragma unroll
  for (int g = 0; g < PB * NX; ++g)
    if (g < kp) {
      const Pack<G> A = Mb[g * 64 + lane];
      G::mfma_pack(A, src[g / PB], PE * (g % PB), acc);
    }
}

// out += M_block' src, M_block a columns-image block ([NX][packs a block][64] packs at `Mb`), src one block of rows
template <typename G, int NX>
__device__ __forceinline__ void times_columns(const Pack<G>* __restrict__ Mb, int lane, const Block<G>& src,
                                              Block<G> (&out)[NX]) {
  constexpr int PB = kPacks<G>, PE = G::Layout::kPack;
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int g = 0; g < PB; ++g) {
      const Pack<G> A = Mb[(ob * PB + g) * 64 + lane];
      G::mfma_pack(A, src, PE * g, out[ob]);
    }
}

template <typename G, int NX>
__device__ __forceinline__ void zero(Block<G> (&x)[NX]) {
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < kRegs<G>; ++i) x[ob][i] = 0;
}

// the sum over a column of a value each lane holds for its rows: the lane groups of a column exchange at the distances
// R, 2 R, .. < 64 in that order (the additions commute: every lane of the column ends with the same bits).  Unrolled by the
// template and not by a loop: a loop leaves the exchanges' lane arithmetic in another order than the straight-line text.
template <typename G, int OFF = kRows<G>>
__device__ __forceinline__ Scalar<G> column_sum(Scalar<G> v) {
  if constexpr (OFF < 64) return column_sum<G, 2 * OFF>(v + __shfl_xor(v, OFF, 64));
  else return v;
}

// the first quadratic of `wave`: the work items (row blocks, then quadratics) go round robin
__device__ __forceinline__ int first_quadratic(int Mb, int wave) { return (wave + kWaves - Mb % kWaves) % kWaves; }

// u = Pe_c p + qe_c, qv = qe_c; returns g_c (the same in every lane of a column)
template <typename G, int NX>
__device__ __forceinline__ Scalar<G> quadratic(const Img<G>& im, int c, int lane, const Block<G> (&p)[NX], Block<G> (&u)[NX],
                                               Block<G> (&qv)[NX]) {
  using T = Scalar<G>;
  constexpr int R = kRows<G>;
  const int grp = lane / R;
#pragma unroll
  for (int ob = 0; ob < NX; ++ob) {
    qv[ob] = G::load_block(im.q + ((size_t)c * NX + ob) * R, grp);
    u[ob] = qv[ob];
    times_rows<G, NX>(im.P + ((size_t)c * NX + ob) * im.kp * 64, im.kp, lane, p, u[ob]);
  }
  T g2 = 0;
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < kRegs<G>; ++i) g2 = fma(p[ob][i], u[ob][i] + qv[ob][i], g2);
  return fma(T(0.5), column_sum<G>(g2), im.r[c]);
}

// This wave's share of the residuals at p: returns max(0, its linear residuals, its g_i) (NaN kept); with GRAD also its
// share of the correction direction, added to `part`.
template <typename G, int NX, bool GRAD>
__device__ __forceinline__ Scalar<G> eval_share(const Img<G>& im, int wave, int lane, const Block<G> (&p)[NX],
                                                Block<G> (&part)[NX]) {
  using T = Scalar<G>;
  constexpr int R = kRows<G>, REGS = kRegs<G>;
  const int grp = lane / R;
  T viol = 0;
  for (int b = wave; b < im.Mb; b += kWaves) {
    Block<G> acc = G::load_block(im.b + (size_t)b * R, grp);
#pragma unroll
    for (int i = 0; i < REGS; ++i) acc[i] = -acc[i];
    times_rows<G, NX>(im.A + (size_t)b * im.kp * 64, im.kp, lane, p, acc);
#pragma unroll
    for (int i = 0; i < REGS; ++i) {
      const T r = acc[i];
      viol = max_nan(viol, r);
      acc[i] = r > T(0) ? r + r : (r != r ? r : T(0));
    }
    if constexpr (GRAD) times_columns<G, NX>(im.AT + (size_t)b * NX * (kPacks<G> * 64), lane, acc, part);
  }
  for (int c = first_quadratic(im.Mb, wave); c < im.nq; c += kWaves) {
    Block<G> u[NX], qv[NX];
    const T g = quadratic<G, NX>(im, c, lane, p, u, qv);
    viol = max_nan(viol, g);
    if constexpr (GRAD) {
      const T gg = g > T(0) ? g + g : (g != g ? g : T(0));
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < REGS; ++i) part[ob][i] = fma(u[ob][i], gg, part[ob][i]);
    }
  }
  return viol;
}

// part += this wave's share of lr J(p)' x   (J of the correction direction at p; rayen_dc3.hip's header)
template <typename G, int NX>
__device__ __forceinline__ void jacobian_transpose_share(const Img<G>& im, int wave, int lane, const Block<G> (&p)[NX],
                                                         const Block<G> (&x)[NX], Scalar<G> lr, Block<G> (&part)[NX]) {
  using T = Scalar<G>;
  constexpr int R = kRows<G>, REGS = kRegs<G>, PB = kPacks<G>, PE = G::Layout::kPack;
  const int grp = lane / R;
  const T lr2 = lr + lr;
  for (int b = wave; b < im.Mb; b += kWaves) {
    Block<G> r = G::load_block(im.b + (size_t)b * R, grp), dx;
#pragma unroll
    for (int i = 0; i < REGS; ++i) {
      r[i] = -r[i];
      dx[i] = 0;
    }
    const Pack<G>* __restrict__ Ab = im.A + (size_t)b * im.kp * 64;
#pragma unroll
    for (int g = 0; g < PB * NX; ++g)
      if (g < im.kp) {
        const Pack<G> A = Ab[g * 64 + lane];
        G::mfma_pack(A, p[g / PB], PE * (g % PB), r);
        G::mfma_pack(A, x[g / PB], PE * (g % PB), dx);
      }
#pragma unroll
    for (int i = 0; i < REGS; ++i) dx[i] = r[i] > T(0) ? lr2 * dx[i] : T(0);
    times_columns<G, NX>(im.AT + (size_t)b * NX * (PB * 64), lane, dx, part);
  }
  for (int c = first_quadratic(im.Mb, wave); c < im.nq; c += kWaves) {
    Block<G> u[NX], qv[NX];
    const T g = quadratic<G, NX>(im, c, lane, p, u, qv);
    T w = 0;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < REGS; ++i) w = fma(u[ob][i], x[ob][i], w);
    w = column_sum<G>(w);
    if (__any(g > T(0))) {
      // 2 (relu(g) Pe' x + [g > 0] w (0.5 (Pe + Pe') p + qe)) = Pe' (2 relu(g) x + [g > 0] w p) + [g > 0] w (u + qe)
      const T cg = g > T(0) ? lr2 * g : T(0);
      const T cw = g > T(0) ? lr * w : T(0);
      Block<G> z[NX];
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < REGS; ++i) z[ob][i] = fma(cg, x[ob][i], cw * p[ob][i]);
#pragma unroll
      for (int ob = 0; ob < NX; ++ob) {
        times_rows<G, NX>(im.PT + ((size_t)c * NX + ob) * im.kp * 64, im.kp, lane, z, part[ob]);
#pragma unroll
        for (int i = 0; i < REGS; ++i) part[ob][i] = fma(cw, u[ob][i] + qv[ob][i], part[ob][i]);
      }
    }
  }
}

// The four waves' partial sums meet in LDS; every wave leaves with the same total.  Two workgroup barriers.
template <typename G, int NX>
__device__ __forceinline__ void sum_partials(Scalar<G>* Pbuf, int wave, int lane, const Block<G> (&part)[NX],
                                             Block<G> (&total)[NX]) {
  constexpr int REGS = kRegs<G>, W = NX * kBlock<G>;       // W: one wave's partial
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < REGS; ++i) Pbuf[((wave * NX + ob) * REGS + i) * 64 + lane] = part[ob][i];
  __syncthreads();
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < REGS; ++i) {
      const int at = (ob * REGS + i) * 64 + lane;
      total[ob][i] = (Pbuf[at] + Pbuf[W + at]) + (Pbuf[2 * W + at] + Pbuf[3 * W + at]);
    }
  __syncthreads();
}

// one step from (p, s): every wave ends with the same new (p, s); returns this wave's share of the violation AT the old p
template <typename G, int NX>
__device__ __forceinline__ Scalar<G> step(const Img<G>& im, Scalar<G>* Pbuf, int wave, int lane, Scalar<G> lr,
                                          Scalar<G> momentum, Block<G> (&p)[NX], Block<G> (&s)[NX]) {
  Block<G> part[NX], grad[NX];
  zero<G, NX>(part);
  const Scalar<G> v = eval_share<G, NX, true>(im, wave, lane, p, part);
  sum_partials<G, NX>(Pbuf, wave, lane, part, grad);
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < kRegs<G>; ++i) {
      s[ob][i] = lr * grad[ob][i] + momentum * s[ob][i];
      p[ob][i] -= s[ob][i];
    }
  return v;
}

// rows of the caller's arrays <-> accumulator layout (columns beyond B: zero in, nothing out)
template <typename G, int NX>
__device__ __forceinline__ void load_rows(const Scalar<G>* __restrict__ row, bool live, int n, int grp, Block<G> (&x)[NX]) {
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < kRegs<G>; ++i) {
      const int j = kRows<G> * ob + row_of<G>(i, grp);
      x[ob][i] = (live && j < n) ? row[j] : Scalar<G>(0);
    }
}

template <typename G, int NX>
__device__ __forceinline__ void load_state(const Scalar<G>* __restrict__ src, bool live, int lane, Block<G> (&x)[NX]) {
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < kRegs<G>; ++i) x[ob][i] = live ? src[(ob * kRegs<G> + i) * 64 + lane] : Scalar<G>(0);
}

template <typename G, int NX>
__device__ __forceinline__ void store_state(Scalar<G>* __restrict__ dst, bool live, int lane, const Block<G> (&x)[NX]) {
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < kRegs<G>; ++i)
      if (live) dst[(ob * kRegs<G> + i) * 64 + lane] = x[ob][i];
}

template <typename G>
struct FwdArgs {
  using T = Scalar<G>;
  Img<G> im;
  const int32_t* perm;
  const T* q;
  int64_t B, ldq;
  T* y;
  int64_t ldy;
  T lr, momentum, eps;
  int max_steps;
  int chunk;                 // >= 0: run chunk `chunk`; -1: the finishing launch
  typename G::Word* viol;    // [max_steps + 1]
  T* state0;                 // [tiles][2 NX][regs][64] each: p then s (nullptr with a single chunk)
  T* state1;
  int32_t* tstar;
  int32_t* nan_flag;
};

template <typename G, int NX>
__global__ __launch_bounds__(kThreads) void forward_kernel(const FwdArgs<G> a) {
  using T = Scalar<G>;
  constexpr int R = kRows<G>, REGS = kRegs<G>, BLOCK = kBlock<G>;
  __shared__ T Pbuf[kWaves * NX * BLOCK];
  __shared__ int sh_t;
  const Img<G>& im = a.im;
  int chunk = a.chunk, nsteps;
  const bool record = chunk >= 0;
  if (record) {
    const int t0 = chunk * kChunk;
    if (threadIdx.x == 0) sh_t = 0;
    __syncthreads();
    for (int t = 1 + (int)threadIdx.x; t <= t0; t += kThreads)
      if (G::from_bits(a.viol[t]) < a.eps) atomicOr(&sh_t, 1);
    __syncthreads();
    if (sh_t) return;                             // an earlier step already met the stop rule: write nothing
    nsteps = a.max_steps - t0 < kChunk ? a.max_steps - t0 : kChunk;
  } else {
    if (threadIdx.x == 0) sh_t = a.max_steps;
    __syncthreads();
    for (int t = 1 + (int)threadIdx.x; t < a.max_steps; t += kThreads)
      if (G::from_bits(a.viol[t]) < a.eps) atomicMin(&sh_t, t);
    __syncthreads();
    const int ts = sh_t;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.tstar = ts;
    chunk = (ts - 1) / kChunk;
    const int t0 = chunk * kChunk;
    const int end = a.max_steps - t0 < kChunk ? a.max_steps : t0 + kChunk;
    if (ts == end) return;                        // that chunk's own y is the answer
    nsteps = ts - t0;
  }
  const int lane = threadIdx.x & 63, grp = lane / R, col = lane % R;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);        // (uniform, and the compiler knows it)
  const int64_t tile = blockIdx.x;
  const int64_t sample = tile * R + col;
  const bool live = sample < a.B;
  const int64_t row = tile * R + (live ? col : 0);      // (a column beyond B points at its tile's first row, never outside)
  const int n = im.n;
  Block<G> p[NX], s[NX];
  if (chunk == 0) {
    load_rows<G, NX>(a.q + row * a.ldq, live, n, grp, p);
    zero<G, NX>(s);
  } else {
    const T* src = ((chunk & 1) ? a.state1 : a.state0) + (size_t)tile * 2 * NX * BLOCK;
    load_state<G, NX>(src, live, lane, p);
    load_state<G, NX>(src + NX * BLOCK, live, lane, s);
  }
  const int t0 = chunk * kChunk;
  for (int st = 0; st < nsteps; ++st) {
    const T v = step<G, NX>(im, Pbuf, wave, lane, a.lr, a.momentum, p, s);
    if (record && st >= 1) record_violation<G>(a.viol + t0 + st, v, live);
  }
  if (record) {
    Block<G> none[NX];
    const T v = eval_share<G, NX, false>(im, wave, lane, p, none);
    record_violation<G>(a.viol + t0 + nsteps, v, live);
    if (wave == 0 && t0 + nsteps < a.max_steps) {
      T* dst = ((chunk & 1) ? a.state0 : a.state1) + (size_t)tile * 2 * NX * BLOCK;
      store_state<G, NX>(dst, live, lane, p);
      store_state<G, NX>(dst + NX * BLOCK, live, lane, s);
    }
  }
  // y[partial] = p (wave 0), y[other] = c0 + C p (the row blocks of C round robin)
  T* __restrict__ yr = a.y + row * a.ldy;
  bool bad = false;
  if (wave == 0) {
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < REGS; ++i) {
        const int j = R * ob + row_of<G>(i, grp);
        if (live && j < n) {
          yr[a.perm[j]] = p[ob][i];
          bad |= p[ob][i] != p[ob][i];
        }
      }
  }
  for (int cb = wave; cb < im.Cb; cb += kWaves) {
    Block<G> acc = G::load_block(im.c0 + (size_t)cb * R, grp);
    times_rows<G, NX>(im.C + (size_t)cb * im.kp * 64, im.kp, lane, p, acc);
#pragma unroll
    for (int i = 0; i < REGS; ++i) {
      const int o = R * cb + row_of<G>(i, grp);
      if (live && o < im.no) {
        yr[a.perm[n + o]] = acc[i];
        bad |= acc[i] != acc[i];
      }
    }
  }
  if (bad && a.nan_flag != nullptr) atomicOr(a.nan_flag, 1);
}

template <typename G>
struct BwdArgs {
  using T = Scalar<G>;
  Img<G> im;
  const int32_t* perm;
  const T* q;
  int64_t B, ldq;
  const T* grad_y;
  int64_t ldg;
  T* grad_q;
  int64_t ldgq;
  T lr, momentum;
  int max_steps;
  const int32_t* tstar;
  T* traj;                   // [max_steps][tiles][NX][regs][64]
};

template <typename G, int NX>
__global__ __launch_bounds__(kThreads) void backward_kernel(const BwdArgs<G> a) {
  using T = Scalar<G>;
  constexpr int R = kRows<G>, REGS = kRegs<G>, BLOCK = kBlock<G>;
  __shared__ T Pbuf[kWaves * NX * BLOCK];
  const Img<G>& im = a.im;
  const int lane = threadIdx.x & 63, grp = lane / R, col = lane % R;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tile = blockIdx.x;
  const int64_t sample = tile * R + col;
  const bool live = sample < a.B;
  const int64_t row = tile * R + (live ? col : 0);      // (a column beyond B points at its tile's first row, never outside)
  const int n = im.n;
  int T_steps = *a.tstar;
  if (T_steps > a.max_steps) T_steps = a.max_steps;
  const size_t tiles = gridDim.x;
  T* traj = a.traj + (size_t)tile * NX * BLOCK;               // step t: + t * tiles * NX * BLOCK
  const size_t tstride = tiles * NX * BLOCK;
  Block<G> p[NX], s[NX], w[NX];
  load_rows<G, NX>(a.q + row * a.ldq, live, n, grp, p);
  zero<G, NX>(s);
  for (int t = 0; t < T_steps; ++t) {
    if (wave == 0) store_state<G, NX>(traj + (size_t)t * tstride, live, lane, p);
    if (t + 1 < T_steps) (void)step<G, NX>(im, Pbuf, wave, lane, a.lr, a.momentum, p, s);
  }
  __syncthreads();           // wave 0's trajectory is read by every wave below
  // pbar_T = grad_y[partial] + C' grad_y[other]; s now holds sbar (zero beyond the last step)
  const T* __restrict__ gy = a.grad_y + row * a.ldg;
#pragma unroll
  for (int ob = 0; ob < NX; ++ob)
#pragma unroll
    for (int i = 0; i < REGS; ++i) {
      const int j = R * ob + row_of<G>(i, grp);
      w[ob][i] = (live && j < n) ? gy[a.perm[j]] : T(0);
    }
  Block<G> part[NX], dj[NX];
  if (im.Cb > 0) {
    zero<G, NX>(part);
    for (int cb = wave; cb < im.Cb; cb += kWaves) {
      Block<G> go;
#pragma unroll
      for (int i = 0; i < REGS; ++i) {
        const int o = R * cb + row_of<G>(i, grp);
        go[i] = (live && o < im.no) ? gy[a.perm[n + o]] : T(0);
      }
      times_columns<G, NX>(im.CT + (size_t)cb * NX * (kPacks<G> * 64), lane, go, part);
    }
    sum_partials<G, NX>(Pbuf, wave, lane, part, dj);
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < REGS; ++i) w[ob][i] += dj[ob][i];
  }
  zero<G, NX>(s);
  for (int t = T_steps - 1; t >= 0; --t) {
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < REGS; ++i) s[ob][i] = a.momentum * s[ob][i] - w[ob][i];
    load_state<G, NX>(traj + (size_t)t * tstride, live, lane, p);
    zero<G, NX>(part);
    jacobian_transpose_share<G, NX>(im, wave, lane, p, s, a.lr, part);
    sum_partials<G, NX>(Pbuf, wave, lane, part, dj);
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < REGS; ++i) w[ob][i] += dj[ob][i];
  }
  if (wave == 0) {
    T* __restrict__ gq = a.grad_q + row * a.ldgq;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < REGS; ++i) {
        const int j = R * ob + row_of<G>(i, grp);
        if (live && j < n) gq[j] = w[ob][i];
      }
  }
}

// ---------------------------------------------------------------------------------------------------------- the host side

inline int n_chunks(int max_steps) { return (max_steps + kChunk - 1) / kChunk; }
template <typename G> size_t n_tiles(int64_t B) { return (size_t)((B + kRows<G> - 1) / kRows<G>); }
template <typename G> size_t n_blocks(const RayenDc3Pack* p) { return (size_t)(p->n + kRows<G> - 1) / kRows<G>; }

// the scratch buffers: viol [max_steps + 1] | with more than one launch of steps, (p, s) in register order twice
enum { kViol = 0, kState0 = 1, kState1 = 2 };
template <typename G>
WsLayout<3> forward_ws(const RayenDc3Pack* p, int64_t B, int max_steps) {
  const size_t state = n_chunks(max_steps) > 1 ? n_tiles<G>(B) * 2 * n_blocks<G>(p) * kBlock<G> : 0;
  return ws_layout<3>(
      {{sizeof(typename G::Word), (size_t)max_steps + 1}, {sizeof(Scalar<G>), state}, {sizeof(Scalar<G>), state}});
}

// the recomputed trajectory [max_steps][tiles][nx][regs][64]
template <typename G>
WsLayout<1> backward_ws(const RayenDc3Pack* p, int64_t B, int max_steps) {
  return ws_layout<1>({{sizeof(Scalar<G>), (size_t)max_steps * n_tiles<G>(B) * n_blocks<G>(p) * kBlock<G>}});
}

template <typename G>
bool served(const RayenDc3Pack* p) {
  return p != nullptr && p->*G::kImage != nullptr && p->perm != nullptr && G::Layout::served(p->n, p->m, p->nq, p->no);
}

// f(std::integral_constant<int, nx>) for nx of 1 .. NX
template <int NX, typename F>
int with_blocks(size_t nx, F&& f) {
  if constexpr (NX > 1)
    if (nx < NX) return with_blocks<NX - 1>(nx, f);
  return f(std::integral_constant<int, NX>());
}

template <typename G, int NX>
int launch_forward(FwdArgs<G> a, hipStream_t stream) {
  const unsigned grid = (unsigned)n_tiles<G>(a.B);
  const int chunks = n_chunks(a.max_steps);
  for (int c = 0; c <= chunks; ++c) {
    a.chunk = c < chunks ? c : -1;
    hipLaunchKernelGGL((forward_kernel<G, NX>), dim3(grid), dim3(kThreads), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return RAYEN_E_LAUNCH;
  }
  return RAYEN_OK;
}

template <typename G, int NX>
int launch_backward(const BwdArgs<G>& a, hipStream_t stream) {
  const unsigned grid = (unsigned)n_tiles<G>(a.B);
  hipLaunchKernelGGL((backward_kernel<G, NX>), dim3(grid), dim3(kThreads), 0, stream, a);
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

// ------------------------------------------------------------------------------- the bodies of the six entry points

template <typename G>
int shape_served(int32_t n, int32_t m, int32_t nq, int32_t no) { return G::Layout::served(n, m, nq, no) ? 1 : 0; }

template <typename G>
int pack_set(RayenDc3Pack* p, const double* A1e, const double* b1e, const double* Pe, const double* qe, const double* re,
             const double* C, const double* c0) {
  if (p == nullptr || (p->m > 0 && (A1e == nullptr || b1e == nullptr)) ||
      (p->nq > 0 && (Pe == nullptr || qe == nullptr || re == nullptr)) || (p->no > 0 && (C == nullptr || c0 == nullptr)))
    return RAYEN_E_BAD_ARG;
  Scalar<G>*& img = p->*G::kImage;
  if (img != nullptr) return RAYEN_OK;
  std::vector<Scalar<G>> h;
  // a shape outside the envelope gets no image: the calls answer RAYEN_E_UNSUPPORTED
  if (!G::Layout::image(p->n, p->m, p->nq, p->no, A1e, b1e, Pe, qe, re, C, c0, &h)) return RAYEN_OK;
  const int rc = check_device(p->device);
  if (rc != RAYEN_OK) return rc;
  if (!upload_image(h, &img)) {
    if (img) (void)hipFree(img);
    img = nullptr;
    return RAYEN_E_ALLOC;
  }
  return RAYEN_OK;
}

template <typename G>
int64_t workspace_bytes(const RayenDc3Pack* p, int64_t B, int32_t max_steps, int32_t backward) {
  if (p == nullptr || B < 0 || max_steps < 1) return -1;
  return (int64_t)(backward ? backward_ws<G>(p, B, max_steps).total : forward_ws<G>(p, B, max_steps).total);
}

template <typename G>
int forward(const RayenDc3Pack* p, const Scalar<G>* q, int64_t B, int64_t ldq, Scalar<G>* y, int64_t ldy, double lr,
            double momentum, double eps, int32_t max_steps, int32_t* tstar, void* ws, int64_t ws_bytes, int32_t* nan_flag,
            void* stream) {
  using T = Scalar<G>;
  if (p == nullptr || B < 0 || max_steps < 1 || tstar == nullptr) return RAYEN_E_BAD_ARG;
  if (B > 0 && (q == nullptr || y == nullptr || ldq < p->n || ldy < p->k)) return RAYEN_E_BAD_ARG;
  if (B > ((int64_t)1 << 31) - kThreads) return RAYEN_E_BAD_ARG;
  if (!served<G>(p)) return RAYEN_E_UNSUPPORTED;
  const WsLayout<3> w = forward_ws<G>(p, B, max_steps);
  if (ws == nullptr || ws_bytes < (int64_t)w.total) return RAYEN_E_BAD_ARG;
  const int rc = check_device(p->device);
  if (rc != RAYEN_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(ws, 0, w.bytes[kViol], s) != hipSuccess) return RAYEN_E_LAUNCH;
  if (B == 0) {
    // an empty batch takes no step (the reference's maximum over nothing raises)
    return hipMemsetAsync(tstar, 0, sizeof(int32_t), s) == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
  }
  FwdArgs<G> a;
  a.im = img_of<G>(p);
  a.perm = p->perm;
  a.q = q; a.B = B; a.ldq = ldq; a.y = y; a.ldy = ldy;
  a.lr = (T)lr; a.momentum = (T)momentum; a.eps = (T)eps;
  a.max_steps = max_steps;
  a.chunk = 0;
  a.viol = w.at<typename G::Word>(ws, kViol);
  a.state0 = w.at<T>(ws, kState0);      // (null with a single chunk)
  a.state1 = w.at<T>(ws, kState1);
  a.tstar = tstar;
  a.nan_flag = nan_flag;
  return with_blocks<G::kMaxNX>(n_blocks<G>(p), [&](auto nx) { return launch_forward<G, nx()>(a, s); });
}

template <typename G>
int backward(const RayenDc3Pack* p, const Scalar<G>* q, int64_t B, int64_t ldq, const Scalar<G>* grad_y, int64_t ldg,
             Scalar<G>* grad_q, int64_t ldgq, double lr, double momentum, int32_t max_steps, const int32_t* tstar, void* ws,
             int64_t ws_bytes, void* stream) {
  using T = Scalar<G>;
  if (p == nullptr || B < 0 || max_steps < 1 || tstar == nullptr) return RAYEN_E_BAD_ARG;
  if (B > 0 && (q == nullptr || grad_y == nullptr || grad_q == nullptr || ldq < p->n || ldg < p->k || ldgq < p->n))
    return RAYEN_E_BAD_ARG;
  if (B > ((int64_t)1 << 31) - kThreads) return RAYEN_E_BAD_ARG;
  if (!served<G>(p)) return RAYEN_E_UNSUPPORTED;
  const WsLayout<1> w = backward_ws<G>(p, B, max_steps);
  if (B > 0 && (ws == nullptr || ws_bytes < (int64_t)w.total)) return RAYEN_E_BAD_ARG;
  const int rc = check_device(p->device);
  if (rc != RAYEN_OK || B == 0) return rc;
  BwdArgs<G> a;
  a.im = img_of<G>(p);
  a.perm = p->perm;
  a.q = q; a.B = B; a.ldq = ldq; a.grad_y = grad_y; a.ldg = ldg; a.grad_q = grad_q; a.ldgq = ldgq;
  a.lr = (T)lr; a.momentum = (T)momentum;
  a.max_steps = max_steps;
  a.tstar = tstar;
  a.traj = w.at<T>(ws, 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_blocks<G::kMaxNX>(n_blocks<G>(p), [&](auto nx) { return launch_backward<G, nx()>(a, s); });
}

}  // namespace dc3_tile
}  // namespace rayen
