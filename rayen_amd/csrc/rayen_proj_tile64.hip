// Batched Euclidean projection onto the constraint set in fp64, 16 samples per workgroup on the fp64 matrix cores: the twins
// of rayen_proj_tile.hip's two kernels (same iteration, same per-row stop, same frozen samples and NaN handling, same
// launches of kChunk iterations, same contract: see that header) on v_mfma_f64_16x16x4_f64, for fp64 inputs on programs
// beyond the fp64 wave kernel's LDS image, its 576 rows and its 32 cones.  Exact fp64 (the differences from the mirror are
// summation order); no PSD block.  rho, sigma, alpha and eps stay double.
//
//     p  = Pi_K(v)
//     xt = Kinv (sigma x + 2 q + w0 + rho G'(2 p - v))
//     r  = G xt + h - p
//     stop, answer xt:   max|r| <= eps (1 + max|p|)  and  max|xt - x| <= eps (1 + max|xt|)
//     x <- x + alpha (xt - x),     v <- v + alpha r
//
// Layout (rayen_dc3_tile64.hip's accumulators, rayen_proj_tile.hip's rows).  One workgroup of four waves owns a tile of 16
// consecutive samples: a sample is a COLUMN of every product.  The host re-lays the m rows into Mp padded rows
// (rayen_proj_tile64_layout.h): blocks of 16 rows, each wave a contiguous range of whole blocks, its CONE blocks first, then
// its ORTHANT blocks; pads are zero orthant rows.  A wave keeps its blocks of v (and of p, later r) in accumulator layout, 4
// doubles a block: lane l, register g of a block is column l & 15, row 4 g + (l >> 4), and the B operand of a K-step is
// B[k = l >> 4][j = l & 15] -- register g of u = 2p - v IS the B operand of K-step g of G'u, the registers of xt are B
// operands of G xt, those of the right-hand side of the Kinv product, with no permutation of k and no cross-lane shuffle.
// The A images (G by row block, G' by the same blocks, Kinv) are in per-lane order, two K-steps a 16-byte piece, and
// STREAMED from global memory (L2-resident); h, w0 and perm are stored in register order too (a lane's four values of a
// block are consecutive).
//
// Cones.  A wave writes its cone blocks of v to its own LDS image ([row][16 samples] doubles); lane (sample, group) then
// walks every fourth cone of the wave over that image, in place, and the blocks are read back as p.  Wave-local: no
// workgroup barrier.  The backward keeps v*'s cone blocks in a second LDS image and a 0/1 bit per orthant row, four bits a
// block.
//
// Across waves go the G'u partial sums (they reuse the cone images' LDS once p is back in registers) and the two stop
// maxima: three workgroup barriers an iteration.  Maxima are taken on the 64-bit patterns of |x| (unsigned order = double
// order, a NaN on top).  Columns of an MFMA do not mix and every sum's order is fixed by the set alone: a row's bits depend
// on the set and on that row's input, never on its tile-mates or on B.
// Envelope: rayen::tile64::served() -- fp64, 1 <= n <= 64, no PSD block, the re-laid rows in 24 (n <= 32) or 20 (n > 32)
// blocks of 16 a wave, the backward's LDS within 160 KiB - 256.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "rayen_proj_pack.h"
#include "rayen_proj_tile64_layout.h"

namespace {

using rayen::tile64::instance_blocks;
using rayen::tile64::instance_nx;
using rayen::tile64::kBlockLds;
using rayen::tile64::kFixedLds;
using rayen::tile64::kWaves;
using rayen::tile64::Layout;
using rayen::tile64::lds_bytes;
using rayen::tile64::parked_of;

constexpr int kThreads = 256;
constexpr int kTile = 16;                     // samples per workgroup
constexpr int kChunk = 32;                    // iterations per launch (rayen_proj.hip's)
constexpr unsigned long long kAbsMask = 0x7fffffffffffffffull;

}  // namespace

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

struct RayenProjTile64 {
  Layout L;
  int n = 0, m = 0, kp = 0, nxs = 0, nxi = 0;
  f64x2 *Gimg = nullptr, *GTimg = nullptr, *Kimg = nullptr;
  double *himg = nullptr, *w0img = nullptr;
  int* perm = nullptr;
  int2* cones = nullptr;
};

namespace {

struct TileArgs {
  const f64x2 *Gimg, *GTimg, *Kimg;
  const double *himg, *w0img;
  const int* perm;
  const int2* cones;
  int n, m, kp, nxs;                           // kp: pairs of K-steps over n (8 columns each); nxs: blocks of 16 of n
  int first_block[kWaves + 1], cone_blocks[kWaves], cone_first[kWaves], cone_count[kWaves];
  int vimg_off[kWaves];                        // LDS, in doubles: a wave's cone image
  int vs_off, c_off, max_off;                  // LDS, in doubles: v*'s images (same offsets inside), 2q + w0, the fixed part
  const double* in;                            // q (forward) or g (backward), [B][ld_in]
  int64_t B, ld_in;
  double* out;                                 // z or grad_q
  int64_t ld_out;
  int32_t* iters;
  double* vstar;                               // [B][m], original row order
  double* xs;                                  // [tiles][NX][4][64]: x between launches
  double* vstate;                              // [tiles][Mp / 16][4][64]: v between launches
  int32_t* status;                             // [16 tiles]: 1 once a sample has finished
  double rho, sigma, alpha, eps;
  int max_iters, chunk;
};

// max over |x| on bit patterns: a NaN is larger than everything and stays
__device__ __forceinline__ unsigned long long absmax(unsigned long long acc, double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x) & kAbsMask;
  return acc > b ? acc : b;
}

__device__ __forceinline__ double bits_to_double(unsigned long long b) { return __longlong_as_double((long long)b); }

// the maximum over the four lane groups that hold a column
__device__ __forceinline__ unsigned long long all_groups(unsigned long long v) {
  unsigned long long o = __shfl_xor(v, 16, 64);
  v = v > o ? v : o;
  o = __shfl_xor(v, 32, 64);
  return v > o ? v : o;
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

#define RAYEN_MFMA2(A, SRC, BASE, ACC)                                                  \
  ACC = __builtin_amdgcn_mfma_f64_16x16x4f64((A).x, (SRC)[(BASE) + 0], ACC, 0, 0, 0);   \
  ACC = __builtin_amdgcn_mfma_f64_16x16x4f64((A).y, (SRC)[(BASE) + 1], ACC, 0, 0, 0)

template <int NB, int NX, bool BWD>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 1))) void tile64_kernel(const TileArgs a) {
  extern __shared__ __align__(16) double tile64_smem[];
  double* L = tile64_smem;
  const int lane = threadIdx.x & 63, grp = lane >> 4, col = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);        // (uniform, and the compiler knows it)
  const int64_t tile = blockIdx.x;
  const int64_t sample = tile * kTile + col;
  const bool live = sample < a.B;
  bool done = !live;
  if (a.chunk > 0) {
    done = done || a.status[sample] != 0;
    if (__all(done)) return;                   // (the same answer in every wave: the tile leaves before it touches an image)
  }
  const int n = a.n, m = a.m, kp = a.kp;
  {
    int4* dst = reinterpret_cast<int4*>(L + a.max_off + kFixedLds / 8);
    const int4* src = reinterpret_cast<const int4*>(a.perm);
    for (int i = threadIdx.x; i < a.first_block[kWaves] * 4; i += kThreads) dst[i] = src[i];
    __syncthreads();
  }
  const int fb0 = a.first_block[wave], nb = a.first_block[wave + 1] - fb0, ncb = a.cone_blocks[wave];
  // the images are the same in every iteration: an index the compiler cannot see through keeps it from hoisting their
  // loads out of the loop (that is the whole of G, G', h and perm in registers: it spills)
  int fb = fb0, kbase = 0;
  const int ncones = a.cone_count[wave];
  const int2* __restrict__ cones = a.cones + a.cone_first[wave];
  double* Vw = L + a.vimg_off[wave];           // this wave's cone image [16 ncb][16]
  double* VSw = Vw + a.vs_off;                 // v*'s (backward)
  double* Cimg = L + a.c_off;                  // [NX][4][64]: 2q + w0 (2 g / max|g|)
  double* Pbuf = L;                            // [4][NX][4][64]: the G'u partial sums (over the cone images)
  unsigned long long* Mx = reinterpret_cast<unsigned long long*>(L + a.max_off);      // [4][2][16]
  int* Same = reinterpret_cast<int*>(L + a.max_off + 128);                            // [4][16]
  const int4* perm4 = reinterpret_cast<const int4*>(L + a.max_off + kFixedLds / 8);   // [Mp] in register order: copied above
  const int t0 = a.chunk * kChunk;
  const int t_end = a.max_iters - t0 < kChunk ? a.max_iters : t0 + kChunk;

  // ---- the input row, and what the right-hand side keeps of it
  f64x4 x[NX];
  double scale = 1.0;
  {
    unsigned long long sm = 0;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 16 * ob + 4 * i + grp;
        x[ob][i] = (live && j < n) ? (a.in + sample * a.ld_in)[j] : 0.0;
        sm = absmax(sm, x[ob][i]);
      }
    if constexpr (BWD) scale = bits_to_double(all_groups(sm));
  }
  bool handed_on = false;
  if constexpr (BWD) {
    // the sample was inside (J = I), or its gradient is zero (or NaN: handed on)
    handed_on = live && (a.iters[sample] == 0 || !(scale > 0.0));
    if (a.chunk == 0 && handed_on && wave == 0) {
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = 16 * ob + 4 * i + grp;
          if (j < n) (a.out + sample * a.ld_out)[j] = x[ob][i];
        }
      if (grp == 0) a.status[sample] = 1;
    }
    done = done || handed_on;
    if (__all(done)) return;
    const double safe = scale > 0.0 ? scale : 1.0;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) x[ob][i] = x[ob][i] / safe;
  }
  if (wave == 0) {
#pragma unroll
    for (int ob = 0; ob < NX; ++ob) {
      f64x2 wlo = {0.0, 0.0}, whi = {0.0, 0.0};
      if constexpr (!BWD) {
        const f64x2* w2 = reinterpret_cast<const f64x2*>(a.w0img + (ob * 4 + grp) * 4);
        wlo = w2[0];
        whi = w2[1];
      }
      Cimg[(ob * 4 + 0) * 64 + lane] = x[ob][0] * 2.0 + wlo.x;
      Cimg[(ob * 4 + 1) * 64 + lane] = x[ob][1] * 2.0 + wlo.y;
      Cimg[(ob * 4 + 2) * 64 + lane] = x[ob][2] * 2.0 + whi.x;
      Cimg[(ob * 4 + 3) * 64 + lane] = x[ob][3] * 2.0 + whi.y;
    }
  }

  constexpr int PK = parked_of(NB), NR = NB - PK;      // blocks NR .. NB - 1 keep p in LDS
  double* Park = L + a.max_off + kFixedLds / 8 + a.first_block[kWaves] * 8 + wave * (PK * 256) + lane;
  f64x4 v[NB], p[NR];
  auto load_p = [&](int b) -> f64x4 {
    if (b < NR) return p[b < NR ? b : 0];
    f64x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = Park[((b - NR) * 4 + i) * 64];
    return r;
  };
  auto store_p = [&](int b, const f64x4& val) {
    if (b < NR) { p[b < NR ? b : 0] = val; return; }
#pragma unroll
    for (int i = 0; i < 4; ++i) Park[((b - NR) * 4 + i) * 64] = val[i];
  };
  uint32_t bits[BWD ? (NB + 7) / 8 : 1];       // backward: v* > 0, four bits a block
  if constexpr (BWD) {
#pragma unroll
    for (int w = 0; w < (NB + 7) / 8; ++w) bits[w] = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b < nb) {
        const int4 pr = perm4[(fb0 + b) * 4 + grp];
        const int rows[4] = {pr.x, pr.y, pr.z, pr.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double vs = (live && rows[e] >= 0) ? a.vstar[sample * m + rows[e]] : 0.0;      // (once a launch)
          bits[b >> 3] |= (vs > 0.0 ? 1u : 0u) << (4 * (b & 7) + e);
          if (b < ncb) VSw[(16 * b + 4 * e + grp) * 16 + col] = vs;
        }
      }
    }
  }

  // acc = G src (+ h) on block b of this wave
  auto times_G = [&](const f64x4 (&src)[NX], int b) -> f64x4 {
    f64x4 acc;
    if constexpr (BWD) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = 0.0;
    } else {
      const f64x2* h2 = reinterpret_cast<const f64x2*>(a.himg + ((size_t)(fb + b) * 4 + grp) * 4);
      const f64x2 lo = h2[0], hi = h2[1];
      acc[0] = lo.x; acc[1] = lo.y; acc[2] = hi.x; acc[3] = hi.y;
    }
#pragma unroll
    for (int gp = 0; gp < 2 * NX; ++gp)
      if (gp < kp) {
        const f64x2 A = (a.Gimg + (size_t)(fb + b) * kp * 64)[gp * 64 + lane];
        RAYEN_MFMA2(A, src[gp >> 1], 2 * (gp & 1), acc);
      }
    return acc;
  };

  // p = Pi_K(v) (forward) or D Pi_K(v*) v (backward)
  auto cone_op = [&]() {
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (b < ncb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) Vw[(16 * b + 4 * i + grp) * 16 + col] = v[b][i];
      }
    wave_sync();
    for (int c = grp; c < ncones; c += 4) {
      const int2 cr = cones[c];
      double* base = Vw + cr.x * 16 + col;
      const int last = cr.y - 1;
      if constexpr (!BWD) {
        double s2 = 0.0;
        for (int r = 0; r < last; ++r) s2 = fma(base[r * 16], base[r * 16], s2);
        const double s = sqrt(s2), t = base[last * 16];
        const bool inside = s <= t, zero = s <= -t;
        const double hf = 0.5 * (s + t);
        const double coef = zero ? 0.0 : hf / s;
        if (!inside) {
          for (int r = 0; r < last; ++r) base[r * 16] = coef * base[r * 16];
          base[last * 16] = zero ? 0.0 : hf;
        }
      } else {
        const double* vsb = VSw + cr.x * 16 + col;
        double s2 = 0.0, dot = 0.0;
        for (int r = 0; r < last; ++r) {
          s2 = fma(vsb[r * 16], vsb[r * 16], s2);
          dot = fma(vsb[r * 16], base[r * 16], dot);
        }
        const double s = sqrt(s2), t = vsb[last * 16];
        const bool inside = s <= t, zero = s <= -t;
        const double inv = s > 0.0 ? 1.0 / s : 0.0;
        const double xd = dot * inv, dt = base[last * 16];
        const double da = 0.5 * (xd + dt), ratio = 0.5 * (s + t) * inv;
        if (!inside) {
          for (int r = 0; r < last; ++r) {
            const double xh = vsb[r * 16] * inv;
            base[r * 16] = zero ? 0.0 : da * xh + ratio * (base[r * 16] - xh * xd);
          }
          base[last * 16] = zero ? 0.0 : da;
        }
      }
    }
    wave_sync();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      f64x4 pb;
      if (b < ncb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) pb[i] = Vw[(16 * b + 4 * i + grp) * 16 + col];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (BWD) pb[i] = ((bits[b >> 3] >> (4 * (b & 7) + i)) & 1u) ? v[b][i] : 0.0;
          else pb[i] = fmax(v[b][i], 0.0);
        }
      }
      store_p(b, pb);
    }
  };

  // v*: un-permuted, of the samples in `which`
  double* vtile = a.vstar + (size_t)tile * kTile * m;   // (uniform; a sample's row is 32-bit offsets from it)
  const uint32_t vrow = (uint32_t)(col * m);
  auto store_vstar = [&](bool which) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (b < nb) {
        const int4 pr = perm4[(fb0 + b) * 4 + grp];
        if (which && pr.x >= 0) vtile[vrow + (uint32_t)pr.x] = v[b][0];
        if (which && pr.y >= 0) vtile[vrow + (uint32_t)pr.y] = v[b][1];
        if (which && pr.z >= 0) vtile[vrow + (uint32_t)pr.z] = v[b][2];
        if (which && pr.w >= 0) vtile[vrow + (uint32_t)pr.w] = v[b][3];
      }
  };
  auto store_out = [&](bool which, const f64x4 (&val)[NX], double mul) {
    if (wave != 0) return;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 16 * ob + 4 * i + grp;
        if (which && j < n) (a.out + sample * a.ld_out)[j] = BWD ? val[ob][i] * mul : val[ob][i];
      }
  };

  double* xs = a.xs + (size_t)tile * NX * 256;
  double* vst = a.vstate + ((size_t)tile * a.first_block[kWaves] + fb0) * 256;
  if (a.chunk == 0) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b < nb) {
        v[b] = times_G(x, b);
        __builtin_amdgcn_sched_barrier(0);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[b][i] = 0.0;
      }
    }
    cone_op();
    // v <- p block by block, noting where they differ (only one of the two stays live: registers).  An inside sample's
    // v* is then stored from p, which equals G q + h there (up to the sign of a zero)
    int differ = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const f64x4 pb = load_p(b);
#pragma unroll
      for (int i = 0; i < 4; ++i) differ |= pb[i] != v[b][i] ? 1 : 0;
      v[b] = pb;
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (!BWD) {
      int same = differ == 0 ? 1 : 0;
      same &= __shfl_xor(same, 16, 64);        // (every lane takes part: no shuffle behind a short circuit)
      same &= __shfl_xor(same, 32, 64);
      if (grp == 0) Same[wave * 16 + col] = same;
      __syncthreads();
      const bool interior = !done && Same[col] != 0 && Same[16 + col] != 0 && Same[32 + col] != 0 && Same[48 + col] != 0;
      if (__any(interior)) {
        // G q + h in K: the sample is inside and answers q
        store_out(interior, x, 1.0);
        store_vstar(interior);
        if (wave == 0 && grp == 0 && interior) { a.iters[sample] = 0; a.status[sample] = 1; }
      }
      done = done || interior;
    }
  } else {
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) x[ob][i] = xs[(ob * 4 + i) * 64 + lane];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) v[b][i] = b < nb ? vst[(b * 4 + i) * 64 + lane] : 0.0;
  }

  bool all_done = __all(done);
  for (int t = t0 + 1; t <= t_end && !all_done; ++t) {
    {
      int opaque;
      asm volatile("s_mov_b32 %0, 0" : "=s"(opaque));
      fb = fb0 + opaque;
      kbase = opaque;
    }
    cone_op();
    __syncthreads();                           // every wave has its p back: the partial sums may take the images' LDS
    // G'u of this wave's rows, u = 2p - v; max|p|
    unsigned long long pm = 0;
    {
      f64x4 wacc[NX];
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < 4; ++i) wacc[ob][i] = 0.0;
#pragma unroll
      for (int b = 0; b < NB; ++b)
        if (b < nb) {
          f64x4 u;
          const f64x4 pb = load_p(b);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            u[i] = (pb[i] + pb[i]) - v[b][i];
            pm = absmax(pm, pb[i]);
          }
#pragma unroll
          for (int ob = 0; ob < NX; ++ob)
            if (ob < a.nxs) {
#pragma unroll
              for (int gp = 0; gp < 2; ++gp) {
                const f64x2 A = (a.GTimg + ((size_t)(fb + b) * a.nxs + ob) * 128)[gp * 64 + lane];
                RAYEN_MFMA2(A, u, 2 * gp, wacc[ob]);
              }
            }
          __builtin_amdgcn_sched_barrier(0);     // (the next block's loads stay behind this one's MFMAs: registers)
        }
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < 4; ++i) Pbuf[((wave * NX + ob) * 4 + i) * 64 + lane] = wacc[ob][i];
    }
    __syncthreads();
    // xt = Kinv (sigma x + (2q + w0) + rho G'u): every wave, identically
    f64x4 xt[NX];
    {
      f64x4 rhs[NX];
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int at = (ob * 4 + i) * 64 + lane;
          const double w = (Pbuf[at] + Pbuf[NX * 256 + at]) + (Pbuf[2 * NX * 256 + at] + Pbuf[3 * NX * 256 + at]);
          rhs[ob][i] = fma(a.rho, w, fma(a.sigma, x[ob][i], Cimg[at]));
          xt[ob][i] = 0.0;
        }
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
        if (ob < a.nxs) {
#pragma unroll
          for (int gp = 0; gp < 2 * NX; ++gp)
            if (gp < kp) {
              const f64x2 A = (a.Kimg + ((size_t)ob * kp + kbase) * 64)[gp * 64 + lane];
              RAYEN_MFMA2(A, rhs[gp >> 1], 2 * (gp & 1), xt[ob]);
            }
        }
    }
    // r = G xt + h - p (kept in p), max|r|
    unsigned long long r1 = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (b < nb) {
        const f64x4 acc = times_G(xt, b);
        f64x4 rb = load_p(b);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          rb[i] = acc[i] - rb[i];
          r1 = absmax(r1, rb[i]);
        }
        store_p(b, rb);
        __builtin_amdgcn_sched_barrier(0);
      }
    r1 = all_groups(r1);
    pm = all_groups(pm);
    if (grp == 0) { Mx[(wave * 2 + 0) * 16 + col] = r1; Mx[(wave * 2 + 1) * 16 + col] = pm; }
    unsigned long long r2 = 0, xm = 0;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        r2 = absmax(r2, xt[ob][i] - x[ob][i]);
        xm = absmax(xm, xt[ob][i]);
      }
    r2 = all_groups(r2);
    xm = all_groups(xm);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const unsigned long long o1 = Mx[(w * 2 + 0) * 16 + col], o2 = Mx[(w * 2 + 1) * 16 + col];
      r1 = r1 > o1 ? r1 : o1;
      pm = pm > o2 ? pm : o2;
    }
    const bool conv = bits_to_double(r1) <= a.eps * (1.0 + bits_to_double(pm)) &&
                      bits_to_double(r2) <= a.eps * (1.0 + bits_to_double(xm));
    const bool stop = !done && (conv || t == a.max_iters);
    if (__any(stop)) {
      store_out(stop, xt, scale);
      if constexpr (!BWD) {
        store_vstar(stop);
        if (wave == 0 && grp == 0 && stop) a.iters[sample] = t;
      }
      if (wave == 0 && grp == 0 && stop) a.status[sample] = 1;
    }
    done = done || stop;
    all_done = __all(done);
    // finished samples are frozen
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (b < nb) {
        const f64x4 rb = load_p(b);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[b][i] = done ? v[b][i] : fma(a.alpha, rb[i], v[b][i]);
      }
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) x[ob][i] = done ? x[ob][i] : fma(a.alpha, xt[ob][i] - x[ob][i], x[ob][i]);
  }
  if (all_done) return;
  if (wave == 0) {
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 4; ++i) xs[(ob * 4 + i) * 64 + lane] = x[ob][i];
    if (a.chunk == 0 && grp == 0 && live && !done) a.status[sample] = 0;
  }
#pragma unroll
  for (int b = 0; b < NB; ++b)
    if (b < nb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) vst[(b * 4 + i) * 64 + lane] = v[b][i];
    }
}

// the scratch buffer: x and v between launches in register order, the finished flags
enum { kTileXs = 0, kTileV = 1, kTileStatus = 2 };
rayen::WsLayout<3> tile_ws(const RayenProjTile64* t, int64_t B) {
  const size_t tiles = (size_t)((B + kTile - 1) / kTile);
  return rayen::ws_layout<3>({{sizeof(double), tiles * t->nxi * 256},
                              {sizeof(double), tiles * (size_t)(t->L.Mp / 16) * 256},
                              {sizeof(int32_t), tiles * kTile}});
}

template <int NB, int NX, bool BWD>
int launch_as(TileArgs a, size_t lds, hipStream_t stream) {
  auto kern = tile64_kernel<NB, NX, BWD>;
  if (!rayen::allow_lds(kern, lds)) return RAYEN_E_LAUNCH;
  const unsigned grid = (unsigned)((a.B + kTile - 1) / kTile);
  const int chunks = (a.max_iters + kChunk - 1) / kChunk;
  for (int c = 0; c < chunks; ++c) {
    a.chunk = c;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, stream, a);
    if (hipGetLastError() != hipSuccess) return RAYEN_E_LAUNCH;
  }
  return RAYEN_OK;
}

// the instances: blocks per wave, blocks of n.  The smallest that holds the set runs.
template <bool BWD>
int launch(int nb, int nxi, const TileArgs& a, size_t lds, hipStream_t s) {
  const int inst = instance_blocks(nb, nxi);
  if (nxi == 2) {
    if (inst == 4) return launch_as<4, 2, BWD>(a, lds, s);
    if (inst == 12) return launch_as<12, 2, BWD>(a, lds, s);
    return launch_as<24, 2, BWD>(a, lds, s);
  }
  if (inst == 4) return launch_as<4, 4, BWD>(a, lds, s);
  if (inst == 12) return launch_as<12, 4, BWD>(a, lds, s);
  return launch_as<20, 4, BWD>(a, lds, s);
}

template <bool BWD>
int run(const RayenProjPack* p, const double* in, int64_t B, int64_t ld_in, double* out, int64_t ld_out, int32_t* iters,
        double* vstar, double eps, int32_t max_iters, void* ws, int64_t ws_bytes, void* stream) {
  if (p == nullptr || B < 0 || max_iters < 1 || !(eps >= 0.0)) return RAYEN_E_BAD_ARG;
  if (B > 0 && (in == nullptr || out == nullptr || iters == nullptr || vstar == nullptr || ld_in < p->n || ld_out < p->n))
    return RAYEN_E_BAD_ARG;
  if (B > ((int64_t)1 << 31) / rayen::tile64::kMaxRows) return RAYEN_E_BAD_ARG;
  const RayenProjTile64* t = p->tile64;
  if (t == nullptr || p->psd_dim != 0 || p->unclaimed != 0) return RAYEN_E_UNSUPPORTED;
  const rayen::WsLayout<3> w = tile_ws(t, B);
  if (B > 0 && (ws == nullptr || ws_bytes < (int64_t)w.total)) return RAYEN_E_BAD_ARG;
  int rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK || B == 0) return rc;
  TileArgs a;
  a.Gimg = t->Gimg; a.GTimg = t->GTimg; a.Kimg = t->Kimg; a.himg = t->himg; a.w0img = t->w0img;
  a.perm = t->perm; a.cones = t->cones;
  a.n = t->n; a.m = t->m; a.kp = t->kp; a.nxs = t->nxs;
  int cone_blocks = 0;
  for (int k = 0; k < kWaves; ++k) {
    a.first_block[k] = t->L.first_block[k];
    a.cone_blocks[k] = t->L.cone_blocks[k];
    a.cone_first[k] = t->L.cone_first[k];
    a.cone_count[k] = t->L.cone_count[k];
    a.vimg_off[k] = cone_blocks * (kBlockLds / 8);
    cone_blocks += t->L.cone_blocks[k];
  }
  a.first_block[kWaves] = t->L.first_block[kWaves];
  const size_t lds = lds_bytes(t->L, t->n, BWD);
  const int shared = (int)(std::max((size_t)cone_blocks * kBlockLds, (size_t)kWaves * t->nxi * kBlockLds) / 8);
  a.vs_off = shared;
  a.c_off = shared + (BWD ? cone_blocks * (kBlockLds / 8) : 0);
  a.max_off = a.c_off + t->nxi * 256;
  a.in = in; a.B = B; a.ld_in = ld_in; a.out = out; a.ld_out = ld_out; a.iters = iters; a.vstar = vstar;
  a.xs = w.at<double>(ws, kTileXs);
  a.vstate = w.at<double>(ws, kTileV);
  a.status = w.at<int32_t>(ws, kTileStatus);
  a.rho = p->rho; a.sigma = p->sigma; a.alpha = p->alpha; a.eps = eps;
  a.max_iters = max_iters;
  a.chunk = 0;
  return launch<BWD>(t->L.nb, t->nxi, a, lds, static_cast<hipStream_t>(stream));
}

}  // namespace

namespace rayen {

RayenProjTile64* proj_tile64_create(const double* G, const double* h, const double* Kinv, const double* w0, int n, int m,
                                    int m_lin, const int32_t* soc_rows, int n_soc) {
  Layout L;
  if (!tile64::served(n, m, m_lin, soc_rows, n_soc, &L)) return nullptr;
  RayenProjTile64* t = new (std::nothrow) RayenProjTile64();
  if (t == nullptr) return nullptr;
  t->L = L;
  t->n = n; t->m = m; t->kp = (n + 7) / 8; t->nxs = (n + 15) / 16; t->nxi = instance_nx(n);
  const int blocks = L.Mp / 16, kp = t->kp, nxs = t->nxs;
  auto g_at = [&](int prow, int colj) -> double {
    const int row = L.perm[prow];
    return (row >= 0 && colj < n) ? G[(size_t)row * n + colj] : 0.0;
  };
  // G by row block: [block][gp][lane] -> G[16 block + (lane & 15)][8 gp + (lane >> 4) + 4 e], e = 0, 1
  std::vector<f64x2> Gi((size_t)blocks * kp * 64), GTi((size_t)blocks * nxs * 2 * 64), Ki((size_t)nxs * kp * 64);
  for (int b = 0; b < blocks; ++b)
    for (int gp = 0; gp < kp; ++gp)
      for (int l = 0; l < 64; ++l) {
        const int r = 16 * b + (l & 15), c = 8 * gp + (l >> 4);
        Gi[((size_t)b * kp + gp) * 64 + l] = f64x2{g_at(r, c), g_at(r, c + 4)};
      }
  // G' by the same blocks: [block][ob][gp][lane] -> G[16 block + 8 gp + (lane >> 4) + 4 e][16 ob + (lane & 15)]
  for (int b = 0; b < blocks; ++b)
    for (int ob = 0; ob < nxs; ++ob)
      for (int gp = 0; gp < 2; ++gp)
        for (int l = 0; l < 64; ++l) {
          const int r = 16 * b + 8 * gp + (l >> 4), c = 16 * ob + (l & 15);
          GTi[(((size_t)b * nxs + ob) * 2 + gp) * 64 + l] = f64x2{g_at(r, c), g_at(r + 4, c)};
        }
  // Kinv: [ob][gp][lane] -> Kinv[k = 8 gp + (lane >> 4) + 4 e][16 ob + (lane & 15)]
  auto k_at = [&](int k, int j) -> double { return (k < n && j < n) ? Kinv[(size_t)k * n + j] : 0.0; };
  for (int ob = 0; ob < nxs; ++ob)
    for (int gp = 0; gp < kp; ++gp)
      for (int l = 0; l < 64; ++l) {
        const int k = 8 * gp + (l >> 4), j = 16 * ob + (l & 15);
        Ki[((size_t)ob * kp + gp) * 64 + l] = f64x2{k_at(k, j), k_at(k + 4, j)};
      }
  // h, perm and w0 in register order: [block][group][g] -> row 16 block + 4 g + group
  std::vector<double> hi((size_t)L.Mp, 0.0), wi(64, 0.0);
  std::vector<int> pi((size_t)L.Mp, -1);
  for (int b = 0; b < blocks; ++b)
    for (int grp = 0; grp < 4; ++grp)
      for (int g = 0; g < 4; ++g) {
        const int row = L.perm[16 * b + 4 * g + grp];
        pi[(b * 4 + grp) * 4 + g] = row;
        if (row >= 0) hi[(b * 4 + grp) * 4 + g] = h[row];
      }
  for (int j = 0; j < n; ++j) wi[((j / 16) * 4 + (j & 3)) * 4 + ((j & 15) >> 2)] = w0[j];
  std::vector<int2> ci(std::max<size_t>(L.cone_rows.size(), 1), make_int2(0, 1));
  for (size_t c = 0; c < L.cone_rows.size(); ++c) ci[c] = make_int2(L.cone_row0[c], L.cone_rows[c]);
  const bool ok = upload_image(Gi, &t->Gimg) && upload_image(GTi, &t->GTimg) && upload_image(Ki, &t->Kimg) &&
                  upload_image(hi, &t->himg) && upload_image(wi, &t->w0img) && upload_image(pi, &t->perm) &&
                  upload_image(ci, &t->cones);
  if (!ok) {
    proj_tile64_destroy(t);
    return nullptr;
  }
  return t;
}

void proj_tile64_destroy(RayenProjTile64* t) {
  if (t == nullptr) return;
  if (t->Gimg) (void)hipFree(t->Gimg);
  if (t->GTimg) (void)hipFree(t->GTimg);
  if (t->Kimg) (void)hipFree(t->Kimg);
  if (t->himg) (void)hipFree(t->himg);
  if (t->w0img) (void)hipFree(t->w0img);
  if (t->perm) (void)hipFree(t->perm);
  if (t->cones) (void)hipFree(t->cones);
  delete t;
}

}  // namespace rayen

extern "C" {

int rayen_proj_tile64_layout(int32_t n, int32_t m_lin, const int32_t* soc_rows, int32_t n_soc, int32_t* Mp, int32_t* perm_out,
                             int32_t* wave_first_block_out, int64_t* lds_bytes_out) {
  if (Mp == nullptr || n < 1 || m_lin < 0 || n_soc < 0 || (n_soc > 0 && soc_rows == nullptr)) return RAYEN_E_BAD_ARG;
  int64_t m = m_lin;
  for (int c = 0; c < n_soc; ++c) {
    if (soc_rows[c] < 1) return RAYEN_E_BAD_ARG;
    m += soc_rows[c];
  }
  if (m < 1) return RAYEN_E_BAD_ARG;
  Layout L;
  if (m > rayen::tile64::kMaxRows || !rayen::tile64::served(n, (int)m, m_lin, soc_rows, n_soc, &L)) return RAYEN_E_UNSUPPORTED;
  *Mp = L.Mp;
  if (perm_out != nullptr) std::memcpy(perm_out, L.perm.data(), sizeof(int32_t) * (size_t)L.Mp);
  if (wave_first_block_out != nullptr) std::memcpy(wave_first_block_out, L.first_block, sizeof(L.first_block));
  if (lds_bytes_out != nullptr) *lds_bytes_out = (int64_t)lds_bytes(L, n, true);
  return RAYEN_OK;
}

int rayen_proj_tile64_pack_set(RayenProjPack* p, const double* G, const double* h, const double* Kinv, const double* w0,
                               const int32_t* soc_rows, int32_t n_soc) {
  if (p == nullptr || G == nullptr || h == nullptr || Kinv == nullptr || w0 == nullptr || n_soc != p->n_soc ||
      (n_soc > 0 && soc_rows == nullptr))
    return RAYEN_E_BAD_ARG;
  if (p->tile64 != nullptr) return RAYEN_OK;
  if (p->psd_dim != 0 || p->unclaimed != 0) return RAYEN_OK;      // a PSD block: no image, the calls answer RAYEN_E_UNSUPPORTED
  Layout L;
  if (!rayen::tile64::served(p->n, p->m, p->m_lin, soc_rows, n_soc, &L)) return RAYEN_OK;
  const int rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK) return rc;
  p->tile64 = rayen::proj_tile64_create(G, h, Kinv, w0, p->n, p->m, p->m_lin, soc_rows, n_soc);
  return p->tile64 != nullptr ? RAYEN_OK : RAYEN_E_ALLOC;
}

int rayen_proj_tile64_served(const RayenProjPack* pack) {
  return pack != nullptr && pack->tile64 != nullptr && pack->psd_dim == 0 && pack->unclaimed == 0;
}

int64_t rayen_proj_tile64_workspace_bytes(const RayenProjPack* pack, int64_t B, int32_t backward) {
  (void)backward;                              // (the same regions either way: the backward keeps v*'s data in LDS)
  if (pack == nullptr || B < 0) return -1;
  if (pack->tile64 == nullptr) return 0;
  return (int64_t)tile_ws(pack->tile64, B).total;
}

int rayen_proj_tile64_forward_f64(const RayenProjPack* pack, const double* q, int64_t B, int64_t ldq, double* z, int64_t ldz,
                                  int32_t* iters, double* vstar, double eps, int32_t max_iters, void* ws, int64_t ws_bytes,
                                  void* stream) {
  return run<false>(pack, q, B, ldq, z, ldz, iters, vstar, eps, max_iters, ws, ws_bytes, stream);
}

int rayen_proj_tile64_backward_f64(const RayenProjPack* pack, const double* g, int64_t B, int64_t ldg, const double* vstar,
                                   const int32_t* iters, double* grad_q, int64_t ldgq, double eps, int32_t max_iters, void* ws,
                                   int64_t ws_bytes, void* stream) {
  return run<true>(pack, g, B, ldg, grad_q, ldgq, const_cast<int32_t*>(iters), const_cast<double*>(vstar), eps, max_iters,
                   ws, ws_bytes, stream);
}

}  // extern "C"
