// Batched Euclidean projection onto the constraint set, 32 samples per workgroup on the matrix cores: the iteration of
// rayen_proj.hip (same mathematics, same per-row stop, same contract) for programs beyond that kernel's LDS image, its 576
// rows and its 32 cones.  Exact fp32 only (v_mfma_f32_32x32x2_f32 is bit for bit an fmaf chain: the differences from the
// mirror are summation order); no PSD block.
//
//     p  = Pi_K(v)
//     xt = Kinv (sigma x + 2 q + w0 + rho G'(2 p - v))
//     r  = G xt + h - p
//     stop, answer xt:   max|r| <= eps (1 + max|p|)  and  max|xt - x| <= eps (1 + max|xt|)
//     x <- x + alpha (xt - x),     v <- v + alpha r
//
// Layout.  One workgroup of four waves (one per SIMD: 512 registers a lane) owns a tile of 32 consecutive samples: a sample
// is a COLUMN of every product.  The host re-lays the m rows into Mp padded rows (tile_layout below): blocks of 32 rows,
// each wave a contiguous range of whole blocks, a wave's CONE blocks first (its cones back to back, then zero pads), then
// its ORTHANT blocks.  A cone never crosses a wave's range; pads are zero orthant rows (G row 0, h 0): they stay at v = 0,
// r = 0.  A wave keeps its blocks of v (and of p, later r) in MFMA accumulator layout, 16 registers a block, for the whole
// launch.  Lane l, register i of a block is column l & 31, row 8 (i >> 2) + 4 (l >> 5) + (i & 3); the B operand of
// 32x32x2_f32 is B[k = l >> 5][j = l & 31]: so register i of u = 2p - v IS the B operand of a k-step of G'u (its half-waves
// hold rows r and r + 4), the registers of xt are B operands of G xt, those of the right-hand side of the Kinv product.  The
// host stores the A images (G by row block, G' by the same blocks, Kinv) with k permuted to match and in per-lane order:
// one coalesced 16-byte load a lane feeds four MFMAs.  The images are STREAMED from global memory (L2-resident: config 5's
// two are 2 x 180 KB); none is held in LDS.  No cross-lane shuffle between the products.
//
// Cones.  A wave writes its cone blocks of v to its own LDS image ([row][32 samples]); lane (sample, half) then walks every
// second cone of the wave over that image -- norm, (s, t), scaling, in place -- and the blocks are read back as p: runtime
// cone boundaries meet runtime LDS addresses, never a register index.  Wave-local: no workgroup barrier.  The backward
// keeps v*'s cone blocks in a second LDS image and a 0/1 bit per orthant row in one register per block.
//
// Across waves go the G'u partial sums (n x 32 a wave; they reuse the cone images' LDS once p is back in registers) and the
// two stop maxima: three workgroup barriers an iteration.  Every wave then forms the right-hand side, xt and the stop
// decision redundantly and identically.  Maxima are taken on the bit patterns of |x| (unsigned order = float order, a NaN
// on top): a NaN sample never meets the stop rule, runs to the cap and answers NaN in its own column; columns of an MFMA
// do not mix, so its 31 tile-mates are neither delayed nor changed.  A finished sample is frozen (answer, iters and v*
// written at its stop, updates masked); a tile whose samples have all finished leaves, at a launch's start before it
// touches an image.  Launches of kChunk iterations; between them (x, v) rest in the caller's workspace in register order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "rayen_proj_pack.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kChunk = 32;                    // iterations per launch (rayen_proj.hip's)
constexpr int kMaxN = 64;
constexpr int kMaxCones = 4096;               // the cone table is device memory: this bounds its size only
constexpr int kBlockLds = 32 * 32 * 4;        // bytes of one block's LDS image
constexpr int kFixedLds = 1024 + 512;         // the stop maxima [4][2][32], the interior flags [4][32]; perm [Mp] follows

// blocks per wave by n: v and p take 32 registers a block, x / xt / G'u 48 a block of n, one accumulator 16.  The instance
// of 12 blocks keeps p of its last 3 blocks (that of 10: 1) in LDS (each lane its own 16 words a block: no synchronisation), or it
// would spill.
inline int max_blocks(int n) { return n <= 32 ? 12 : 10; }
constexpr int parked_of(int NB) { return NB > 10 ? 3 : NB == 10 ? 1 : 0; }
inline int instance_blocks(int nb, int nx) { return nb <= 2 ? 2 : nb <= 6 ? 6 : nx == 1 ? 12 : 10; }

struct Layout {
  int Mp = 0, nb = 0;                         // padded rows; blocks of the fullest wave
  int first_block[kWaves + 1] = {};
  int cone_blocks[kWaves] = {}, cone_first[kWaves] = {}, cone_count[kWaves] = {};
  std::vector<int> perm;                      // [Mp]: original row, -1 for a pad
  std::vector<int> cone_row0, cone_rows;      // per cone: first row inside its wave's cone image, rows
};

// The re-laying of the rows (tests/tile_layout_formulas.py restates it).  nb = the smallest number of blocks per wave at
// which this holds: the cones, in order, go to waves 0, 1, .. (a cone that no longer fits the wave's 32 nb rows opens the
// next wave); the orthant rows then fill the blocks the cones left, wave 0 first.  false: no nb <= nb_limit holds them.
bool tile_layout(int m_lin, const int32_t* soc_rows, int n_soc, int nb_limit, Layout* out) {
  for (int nb = 1; nb <= nb_limit; ++nb) {
    const int cap = 32 * nb;
    int used[kWaves] = {}, count[kWaves] = {}, w = 0;
    bool ok = true;
    for (int c = 0; c < n_soc && ok; ++c) {
      while (w < kWaves && used[w] + soc_rows[c] > cap) ++w;
      if (w == kWaves) { ok = false; break; }
      used[w] += soc_rows[c];
      ++count[w];
    }
    if (!ok) continue;
    int64_t room = 0;
    for (int k = 0; k < kWaves; ++k) room += cap - 32 * ((used[k] + 31) / 32);
    if (room < m_lin) continue;
    Layout& L = *out;
    L = Layout();
    L.nb = nb;
    int cone = 0, orth = 0, at = 0;
    for (int k = 0; k < kWaves; ++k) {
      L.first_block[k] = at / 32;
      L.cone_blocks[k] = (used[k] + 31) / 32;
      L.cone_first[k] = cone;
      L.cone_count[k] = count[k];
      int local = 0;
      for (int c = 0; c < count[k]; ++c, ++cone) {
        L.cone_row0.push_back(local);
        L.cone_rows.push_back(soc_rows[cone]);
        for (int r = 0; r < soc_rows[cone]; ++r) L.perm.push_back(-2);      // (numbered below: the cones follow the orthant rows)
        local += soc_rows[cone];
      }
      for (; local < 32 * L.cone_blocks[k]; ++local) L.perm.push_back(-1);
      const int take = std::min(m_lin - orth, cap - 32 * L.cone_blocks[k]);
      for (int r = 0; r < take; ++r) L.perm.push_back(orth++);
      for (int r = take; r % 32 != 0; ++r) L.perm.push_back(-1);
      at = (int)L.perm.size();
    }
    L.first_block[kWaves] = at / 32;
    L.Mp = at;
    int row = m_lin;
    for (int& p : L.perm)
      if (p == -2) p = row++;
    return true;
  }
  return false;
}

size_t lds_bytes(const Layout& L, int n, bool backward) {
  const int nx = (n + 31) / 32;
  const size_t parked = (size_t)kWaves * parked_of(instance_blocks(L.nb, nx)) * 16 * 64 * 4;
  int cone_blocks = 0;
  for (int k = 0; k < kWaves; ++k) cone_blocks += L.cone_blocks[k];
  const size_t shared = std::max((size_t)cone_blocks * kBlockLds, (size_t)kWaves * nx * 16 * 64 * 4);
  return shared + (backward ? (size_t)cone_blocks * kBlockLds : 0) + (size_t)nx * 16 * 64 * 4 + kFixedLds + (size_t)L.Mp * 4 + parked;
}

// tile_served(): the one rule.  n in two blocks of x; the rows, re-laid, in max_blocks(n) blocks a wave (the register
// file); the cone blocks' images (twice: the backward's v*), the partial sums and 2q + w0 in LDS.  Forward and backward
// serve the same sets: the rule is the backward's.
bool tile_served(int n, int m, int m_lin, const int32_t* soc_rows, int n_soc, Layout* L) {
  if (n < 1 || n > kMaxN || m < 1 || n_soc < 0 || n_soc > kMaxCones || m_lin < 0) return false;
  int64_t rows = m_lin;
  for (int c = 0; c < n_soc; ++c) {
    if (soc_rows[c] < 1) return false;
    rows += soc_rows[c];
  }
  if (rows != m) return false;                                    // (rows left over: a PSD block)
  if (rows > 4 * 32 * 12) return false;
  if (!tile_layout(m_lin, soc_rows, n_soc, max_blocks(n), L)) return false;
  return lds_bytes(*L, n, true) <= rayen::kLdsBudget - 256;
}

}  // namespace

struct RayenProjTile {
  Layout L;
  int n = 0, m = 0, kg = 0, nx = 0;
  float4 *Gimg = nullptr, *GTimg = nullptr, *Kimg = nullptr;
  float *himg = nullptr, *w0img = nullptr;
  int* perm = nullptr;
  int2* cones = nullptr;
};

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct TileArgs {
  const float4 *Gimg, *GTimg, *Kimg;
  const float *himg, *w0img;
  const int* perm;
  const int2* cones;
  int n, m, kg, nxs;                           // kg: groups of 8 columns of n; nxs: blocks of 32 of n
  int first_block[kWaves + 1], cone_blocks[kWaves], cone_first[kWaves], cone_count[kWaves];
  int vimg_off[kWaves];                        // LDS, in floats: a wave's cone image
  int vs_off, c_off, max_off;                  // LDS, in floats: v*'s images (same offsets inside), 2q + w0, the fixed part
  const float* in;                             // q (forward) or g (backward), [B][ld_in]
  int64_t B, ld_in;
  float* out;                                  // z or grad_q
  int64_t ld_out;
  int32_t* iters;
  float* vstar;                                // [B][m], original row order
  float* xs;                                   // [tiles][nx][16][64]: x between launches
  float* vstate;                               // [tiles][Mp / 32][16][64]: v between launches
  int32_t* status;                             // [B]: 1 once a sample has finished
  float rho, sigma, alpha, eps;
  int max_iters, chunk;
};

__device__ __forceinline__ int row_of(int i, int half) { return 8 * (i >> 2) + 4 * half + (i & 3); }

// max over |x| on bit patterns: a NaN is larger than everything and stays
__device__ __forceinline__ uint32_t absmax(uint32_t acc, float x) {
  const uint32_t b = __float_as_uint(x) & 0x7fffffffu;
  return acc > b ? acc : b;
}

__device__ __forceinline__ uint32_t both_halves(uint32_t v) {
  const uint32_t o = (uint32_t)__shfl_xor((int)v, 32, 64);
  return v > o ? v : o;
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

#define RAYEN_MFMA4(A, SRC, BASE, ACC)                                           \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).x, (SRC)[(BASE) + 0], ACC, 0, 0, 0); \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).y, (SRC)[(BASE) + 1], ACC, 0, 0, 0); \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).z, (SRC)[(BASE) + 2], ACC, 0, 0, 0); \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).w, (SRC)[(BASE) + 3], ACC, 0, 0, 0)

template <int NB, int NX, bool BWD>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 1))) void tile_kernel(const TileArgs a) {
  extern __shared__ __align__(16) float tile_smem[];
  float* L = tile_smem;
  const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);        // (uniform, and the compiler knows it)
  const int64_t tile = blockIdx.x;
  const int64_t sample = tile * 32 + col;
  const bool live = sample < a.B;
  bool done = !live;
  if (a.chunk > 0) {
    done = done || a.status[sample] != 0;
    if (__all(done)) return;                   // (the same answer in every wave: the tile leaves before it touches an image)
  }
  const int n = a.n, m = a.m, kg = a.kg;
  {
    int4* dst = reinterpret_cast<int4*>(L + a.max_off + kFixedLds / 4);
    const int4* src = reinterpret_cast<const int4*>(a.perm);
    for (int i = threadIdx.x; i < a.first_block[kWaves] * 8; i += kThreads) dst[i] = src[i];
    __syncthreads();
  }
  const int fb0 = a.first_block[wave], nb = a.first_block[wave + 1] - fb0, ncb = a.cone_blocks[wave];
  // the images are the same in every iteration: an index the compiler cannot see through keeps it from hoisting their
  // loads out of the loop (that is the whole of G, G', h and perm in registers: it spills)
  int fb = fb0, kbase = 0;
  const int ncones = a.cone_count[wave];
  const int2* __restrict__ cones = a.cones + a.cone_first[wave];
  float* Vw = L + a.vimg_off[wave];            // this wave's cone image [32 ncb][32]
  float* VSw = Vw + a.vs_off;                  // v*'s (backward)
  float* Cimg = L + a.c_off;                   // [NX][16][64]: 2q + w0 (2 g / max|g|)
  float* Pbuf = L;                             // [4][NX][16][64]: the G'u partial sums (over the cone images)
  uint32_t* Mx = reinterpret_cast<uint32_t*>(L + a.max_off);      // [4][2][32]
  int* Same = reinterpret_cast<int*>(L + a.max_off) + 256;        // [4][32]
  const float4* __restrict__ h4 = reinterpret_cast<const float4*>(a.himg);
  const int4* perm4 = reinterpret_cast<const int4*>(L + a.max_off + kFixedLds / 4);      // [Mp]: copied below
  const int t0 = a.chunk * kChunk;
  const int t_end = a.max_iters - t0 < kChunk ? a.max_iters : t0 + kChunk;

  // ---- the input row, and what the right-hand side keeps of it
  f32x16 x[NX];
  float scale = 1.0f;
  {
    uint32_t sm = 0;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int j = 32 * ob + row_of(i, half);
        x[ob][i] = (live && j < n) ? (a.in + sample * a.ld_in + 4 * half)[32 * ob + row_of(i, 0)] : 0.0f;
        sm = absmax(sm, x[ob][i]);
      }
    if constexpr (BWD) scale = __uint_as_float(both_halves(sm));
  }
  bool handed_on = false;
  if constexpr (BWD) {
    // the sample was inside (J = I), or its gradient is zero (or NaN: handed on)
    handed_on = live && (a.iters[sample] == 0 || !(scale > 0.0f));
    if (a.chunk == 0 && handed_on && wave == 0) {
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int j = 32 * ob + row_of(i, half);
          if (j < n) (a.out + sample * a.ld_out + 4 * half)[32 * ob + row_of(i, 0)] = x[ob][i];
        }
      if (half == 0) a.status[sample] = 1;
    }
    done = done || handed_on;
    if (__all(done)) return;
    const float safe = scale > 0.0f ? scale : 1.0f;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 16; ++i) x[ob][i] = x[ob][i] / safe;
  }
  if (wave == 0) {
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 w0 = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (!BWD) w0 = reinterpret_cast<const float4*>(a.w0img)[(32 * ob + 8 * g + 4 * half) / 4];
        Cimg[(ob * 16 + 4 * g + 0) * 64 + lane] = x[ob][4 * g + 0] * 2.0f + w0.x;
        Cimg[(ob * 16 + 4 * g + 1) * 64 + lane] = x[ob][4 * g + 1] * 2.0f + w0.y;
        Cimg[(ob * 16 + 4 * g + 2) * 64 + lane] = x[ob][4 * g + 2] * 2.0f + w0.z;
        Cimg[(ob * 16 + 4 * g + 3) * 64 + lane] = x[ob][4 * g + 3] * 2.0f + w0.w;
      }
  }

  constexpr int PK = parked_of(NB), NR = NB - PK;      // blocks NR .. NB - 1 keep p in LDS
  float* Park = L + a.max_off + kFixedLds / 4 + a.first_block[kWaves] * 32 + wave * (PK * 1024) + lane;
  f32x16 v[NB], p[NB];
  auto load_p = [&](int b) -> f32x16 {
    if (b < NR) return p[b];
    f32x16 r;
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = Park[((b - NR) * 16 + i) * 64];
    return r;
  };
  auto store_p = [&](int b, const f32x16& val) {
    if (b < NR) { p[b] = val; return; }
#pragma unroll
    for (int i = 0; i < 16; ++i) Park[((b - NR) * 16 + i) * 64] = val[i];
  };
  uint32_t bits[BWD ? NB : 1];                 // backward: v* > 0, one bit per register of a block
  if constexpr (BWD) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      bits[b] = 0;
      if (b < nb) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int4 pr = (perm4 + (fb0 + b) * 8)[2 * g + half];
          const int rows[4] = {pr.x, pr.y, pr.z, pr.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float vs = (live && rows[e] >= 0) ? a.vstar[sample * m + rows[e]] : 0.0f;      // (once a launch)
            bits[b] |= (vs > 0.0f ? 1u : 0u) << (4 * g + e);
            if (b < ncb) VSw[(32 * b + row_of(4 * g + e, half)) * 32 + col] = vs;
          }
        }
      }
    }
  }

  // acc = G src (+ h) on block b of this wave
  auto times_G = [&](const f32x16 (&src)[NX], int b) -> f32x16 {
    f32x16 acc;
    if constexpr (BWD) {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 hv = (h4 + (fb + b) * 8)[2 * g + half];
        acc[4 * g + 0] = hv.x; acc[4 * g + 1] = hv.y; acc[4 * g + 2] = hv.z; acc[4 * g + 3] = hv.w;
      }
    }
#pragma unroll
    for (int g = 0; g < 4 * NX; ++g)
      if (g < kg) {
        const float4 A = (a.Gimg + (size_t)(fb + b) * kg * 64)[g * 64 + lane];
        RAYEN_MFMA4(A, src[g >> 2], 4 * (g & 3), acc);
      }
    return acc;
  };

  // p = Pi_K(v) (forward) or D Pi_K(v*) v (backward)
  auto cone_op = [&]() {
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (b < ncb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) Vw[(32 * b + row_of(i, half)) * 32 + col] = v[b][i];
      }
    wave_sync();
    for (int c = half; c < ncones; c += 2) {
      const int2 cr = cones[c];
      float* base = Vw + cr.x * 32 + col;
      const int last = cr.y - 1;
      if constexpr (!BWD) {
        float s2 = 0.0f;
        for (int r = 0; r < last; ++r) s2 = fmaf(base[r * 32], base[r * 32], s2);
        const float s = sqrtf(s2), t = base[last * 32];
        const bool inside = s <= t, zero = s <= -t;
        const float hf = 0.5f * (s + t);
        const float coef = zero ? 0.0f : hf / s;
        if (!inside) {
          for (int r = 0; r < last; ++r) base[r * 32] = coef * base[r * 32];
          base[last * 32] = zero ? 0.0f : hf;
        }
      } else {
        const float* vsb = VSw + cr.x * 32 + col;
        float s2 = 0.0f, dot = 0.0f;
        for (int r = 0; r < last; ++r) {
          s2 = fmaf(vsb[r * 32], vsb[r * 32], s2);
          dot = fmaf(vsb[r * 32], base[r * 32], dot);
        }
        const float s = sqrtf(s2), t = vsb[last * 32];
        const bool inside = s <= t, zero = s <= -t;
        const float inv = s > 0.0f ? 1.0f / s : 0.0f;
        const float xd = dot * inv, dt = base[last * 32];
        const float da = 0.5f * (xd + dt), ratio = 0.5f * (s + t) * inv;
        if (!inside) {
          for (int r = 0; r < last; ++r) {
            const float xh = vsb[r * 32] * inv;
            base[r * 32] = zero ? 0.0f : da * xh + ratio * (base[r * 32] - xh * xd);
          }
          base[last * 32] = zero ? 0.0f : da;
        }
      }
    }
    wave_sync();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      f32x16 pb;
      if (b < ncb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) pb[i] = Vw[(32 * b + row_of(i, half)) * 32 + col];
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if constexpr (BWD) pb[i] = ((bits[b] >> i) & 1u) ? v[b][i] : 0.0f;
          else pb[i] = fmaxf(v[b][i], 0.0f);
        }
      }
      store_p(b, pb);
    }
  };

  // v*: un-permuted, of the samples in `which`
  float* vtile = a.vstar + (size_t)tile * 32 * m;       // (uniform; a sample's row is 32-bit offsets from it)
  const uint32_t vrow = (uint32_t)(col * m);
  auto store_vstar = [&](bool which) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (b < nb) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int4 pr = (perm4 + (fb0 + b) * 8)[2 * g + half];
          if (which && pr.x >= 0) vtile[vrow + (uint32_t)pr.x] = v[b][4 * g + 0];
          if (which && pr.y >= 0) vtile[vrow + (uint32_t)pr.y] = v[b][4 * g + 1];
          if (which && pr.z >= 0) vtile[vrow + (uint32_t)pr.z] = v[b][4 * g + 2];
          if (which && pr.w >= 0) vtile[vrow + (uint32_t)pr.w] = v[b][4 * g + 3];
        }
      }
  };
  auto store_out = [&](bool which, const f32x16 (&val)[NX], float mul) {
    if (wave != 0) return;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int j = 32 * ob + row_of(i, half);
        if (which && j < n) (a.out + sample * a.ld_out + 4 * half)[32 * ob + row_of(i, 0)] = BWD ? val[ob][i] * mul : val[ob][i];
      }
  };

  float* xs = a.xs + (size_t)tile * NX * 16 * 64;
  float* vst = a.vstate + ((size_t)tile * a.first_block[kWaves] + fb0) * 16 * 64;
  if (a.chunk == 0) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b < nb) {
        v[b] = times_G(x, b);
        __builtin_amdgcn_sched_barrier(0);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[b][i] = 0.0f;
      }
    }
    cone_op();
    // v <- p block by block, noting where they differ (only one of the two stays live: registers).  An inside sample's
    // v* is then stored from p, which equals G q + h there (up to the sign of a zero)
    int differ = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const f32x16 pb = load_p(b);
#pragma unroll
      for (int i = 0; i < 16; ++i) differ |= pb[i] != v[b][i] ? 1 : 0;
      v[b] = pb;
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (!BWD) {
      bool same = differ == 0;
      const int other = __shfl_xor((int)same, 32, 64);      // (every lane takes part: no shuffle behind a short circuit)
      same = same && other != 0;
      if (half == 0) Same[wave * 32 + col] = same ? 1 : 0;
      __syncthreads();
      const bool interior = !done && Same[col] != 0 && Same[32 + col] != 0 && Same[64 + col] != 0 && Same[96 + col] != 0;
      if (__any(interior)) {
        // G q + h in K: the sample is inside and answers q
        store_out(interior, x, 1.0f);
        store_vstar(interior);
        if (wave == 0 && half == 0 && interior) { a.iters[sample] = 0; a.status[sample] = 1; }
      }
      done = done || interior;
    }
  } else {
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 16; ++i) x[ob][i] = xs[(ob * 16 + i) * 64 + lane];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) v[b][i] = b < nb ? vst[(b * 16 + i) * 64 + lane] : 0.0f;
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
    uint32_t pm = 0;
    {
      f32x16 wacc[NX];
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < 16; ++i) wacc[ob][i] = 0.0f;
#pragma unroll
      for (int b = 0; b < NB; ++b)
        if (b < nb) {
          f32x16 u;
          const f32x16 pb = load_p(b);
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            u[i] = (pb[i] + pb[i]) - v[b][i];
            pm = absmax(pm, pb[i]);
          }
#pragma unroll
          for (int ob = 0; ob < NX; ++ob)
            if (ob < a.nxs) {
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                const float4 A = (a.GTimg + ((size_t)(fb + b) * a.nxs + ob) * 256)[g * 64 + lane];
                RAYEN_MFMA4(A, u, 4 * g, wacc[ob]);
              }
            }
          __builtin_amdgcn_sched_barrier(0);     // (the next block's loads stay behind this one's MFMAs: registers)
        }
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < 16; ++i) Pbuf[((wave * NX + ob) * 16 + i) * 64 + lane] = wacc[ob][i];
    }
    __syncthreads();
    // xt = Kinv (sigma x + (2q + w0) + rho G'u): every wave, identically
    f32x16 xt[NX];
    {
      f32x16 rhs[NX];
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int at = (ob * 16 + i) * 64 + lane;
          const float w = (Pbuf[at] + Pbuf[NX * 1024 + at]) + (Pbuf[2 * NX * 1024 + at] + Pbuf[3 * NX * 1024 + at]);
          rhs[ob][i] = fmaf(a.rho, w, fmaf(a.sigma, x[ob][i], Cimg[at]));
          xt[ob][i] = 0.0f;
        }
#pragma unroll
      for (int ob = 0; ob < NX; ++ob)
        if (ob < a.nxs) {
#pragma unroll
          for (int g = 0; g < 4 * NX; ++g)
            if (g < kg) {
              const float4 A = (a.Kimg + ((size_t)ob * kg + kbase) * 64)[g * 64 + lane];
              RAYEN_MFMA4(A, rhs[g >> 2], 4 * (g & 3), xt[ob]);
            }
        }
    }
    // r = G xt + h - p (kept in p), max|r|
    uint32_t r1 = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (b < nb) {
        const f32x16 acc = times_G(xt, b);
        f32x16 rb = load_p(b);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          rb[i] = acc[i] - rb[i];
          r1 = absmax(r1, rb[i]);
        }
        store_p(b, rb);
        __builtin_amdgcn_sched_barrier(0);
      }
    r1 = both_halves(r1);
    pm = both_halves(pm);
    if (half == 0) { Mx[(wave * 2 + 0) * 32 + col] = r1; Mx[(wave * 2 + 1) * 32 + col] = pm; }
    uint32_t r2 = 0, xm = 0;
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        r2 = absmax(r2, xt[ob][i] - x[ob][i]);
        xm = absmax(xm, xt[ob][i]);
      }
    r2 = both_halves(r2);
    xm = both_halves(xm);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const uint32_t o1 = Mx[(w * 2 + 0) * 32 + col], o2 = Mx[(w * 2 + 1) * 32 + col];
      r1 = r1 > o1 ? r1 : o1;
      pm = pm > o2 ? pm : o2;
    }
    const bool conv = __uint_as_float(r1) <= a.eps * (1.0f + __uint_as_float(pm)) &&
                      __uint_as_float(r2) <= a.eps * (1.0f + __uint_as_float(xm));
    const bool stop = !done && (conv || t == a.max_iters);
    if (__any(stop)) {
      store_out(stop, xt, scale);
      if constexpr (!BWD) {
        store_vstar(stop);
        if (wave == 0 && half == 0 && stop) a.iters[sample] = t;
      }
      if (wave == 0 && half == 0 && stop) a.status[sample] = 1;
    }
    done = done || stop;
    all_done = __all(done);
    // finished samples are frozen
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (b < nb) {
        const f32x16 rb = load_p(b);
#pragma unroll
        for (int i = 0; i < 16; ++i) v[b][i] = done ? v[b][i] : fmaf(a.alpha, rb[i], v[b][i]);
      }
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 16; ++i) x[ob][i] = done ? x[ob][i] : fmaf(a.alpha, xt[ob][i] - x[ob][i], x[ob][i]);
  }
  if (all_done) return;
  if (wave == 0) {
#pragma unroll
    for (int ob = 0; ob < NX; ++ob)
#pragma unroll
      for (int i = 0; i < 16; ++i) xs[(ob * 16 + i) * 64 + lane] = x[ob][i];
    if (a.chunk == 0 && half == 0 && live && !done) a.status[sample] = 0;
  }
#pragma unroll
  for (int b = 0; b < NB; ++b)
    if (b < nb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) vst[(b * 16 + i) * 64 + lane] = v[b][i];
    }
}

// the scratch buffer: x and v between launches in register order, the finished flags
enum { kTileXs = 0, kTileV = 1, kTileStatus = 2 };
rayen::WsLayout<3> tile_ws(const RayenProjTile* t, int64_t B) {
  const size_t tiles = (size_t)((B + 31) / 32);
  return rayen::ws_layout<3>({{sizeof(float), tiles * t->nx * 16 * 64},
                              {sizeof(float), tiles * (size_t)(t->L.Mp / 32) * 16 * 64},
                              {sizeof(int32_t), tiles * 32}});
}

template <int NB, int NX, bool BWD>
int launch_as(TileArgs a, size_t lds, hipStream_t stream) {
  auto kern = tile_kernel<NB, NX, BWD>;
  if (!rayen::allow_lds(kern, lds)) return RAYEN_E_LAUNCH;
  const unsigned grid = (unsigned)((a.B + 31) / 32);
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
int launch(int nb, int nx, const TileArgs& a, size_t lds, hipStream_t s) {
  const int inst = instance_blocks(nb, nx);
  if (nx == 1) {
    if (inst == 2) return launch_as<2, 1, BWD>(a, lds, s);
    if (inst == 6) return launch_as<6, 1, BWD>(a, lds, s);
    return launch_as<12, 1, BWD>(a, lds, s);
  }
  if (inst == 2) return launch_as<2, 2, BWD>(a, lds, s);
  if (inst == 6) return launch_as<6, 2, BWD>(a, lds, s);
  return launch_as<10, 2, BWD>(a, lds, s);
}

template <bool BWD>
int run(const RayenProjPack* p, const float* in, int64_t B, int64_t ld_in, float* out, int64_t ld_out, int32_t* iters,
        float* vstar, double eps, int32_t max_iters, void* ws, int64_t ws_bytes, void* stream) {
  if (p == nullptr || B < 0 || max_iters < 1 || !(eps >= 0.0)) return RAYEN_E_BAD_ARG;
  if (B > 0 && (in == nullptr || out == nullptr || iters == nullptr || vstar == nullptr || ld_in < p->n || ld_out < p->n))
    return RAYEN_E_BAD_ARG;
  if (B > ((int64_t)1 << 31) / (4 * 32 * 12)) return RAYEN_E_BAD_ARG;
  const RayenProjTile* t = p->tile;
  if (t == nullptr || p->psd_dim != 0 || p->unclaimed != 0) return RAYEN_E_UNSUPPORTED;
  const rayen::WsLayout<3> w = tile_ws(t, B);
  if (B > 0 && (ws == nullptr || ws_bytes < (int64_t)w.total)) return RAYEN_E_BAD_ARG;
  int rc = rayen::check_device(p->device);
  if (rc != RAYEN_OK || B == 0) return rc;
  TileArgs a;
  a.Gimg = t->Gimg; a.GTimg = t->GTimg; a.Kimg = t->Kimg; a.himg = t->himg; a.w0img = t->w0img;
  a.perm = t->perm; a.cones = t->cones;
  a.n = t->n; a.m = t->m; a.kg = t->kg; a.nxs = t->nx;
  int cone_blocks = 0;
  for (int k = 0; k < kWaves; ++k) {
    a.first_block[k] = t->L.first_block[k];
    a.cone_blocks[k] = t->L.cone_blocks[k];
    a.cone_first[k] = t->L.cone_first[k];
    a.cone_count[k] = t->L.cone_count[k];
    a.vimg_off[k] = cone_blocks * (kBlockLds / 4);
    cone_blocks += t->L.cone_blocks[k];
  }
  a.first_block[kWaves] = t->L.first_block[kWaves];
  const size_t lds = lds_bytes(t->L, t->n, BWD);
  const int shared = (int)(std::max((size_t)cone_blocks * kBlockLds, (size_t)kWaves * t->nx * 16 * 64 * 4) / 4);
  a.vs_off = shared;
  a.c_off = shared + (BWD ? cone_blocks * (kBlockLds / 4) : 0);
  a.max_off = a.c_off + t->nx * 16 * 64;
  a.in = in; a.B = B; a.ld_in = ld_in; a.out = out; a.ld_out = ld_out; a.iters = iters; a.vstar = vstar;
  a.xs = w.at<float>(ws, kTileXs);
  a.vstate = w.at<float>(ws, kTileV);
  a.status = w.at<int32_t>(ws, kTileStatus);
  a.rho = (float)p->rho; a.sigma = (float)p->sigma; a.alpha = (float)p->alpha; a.eps = (float)eps;
  a.max_iters = max_iters;
  a.chunk = 0;
  return launch<BWD>(t->L.nb, t->nx, a, lds, static_cast<hipStream_t>(stream));
}

}  // namespace

namespace rayen {

RayenProjTile* proj_tile_create(const double* G, const double* h, const double* Kinv, const double* w0, int n, int m,
                                int m_lin, const int32_t* soc_rows, int n_soc) {
  Layout L;
  if (!tile_served(n, m, m_lin, soc_rows, n_soc, &L)) return nullptr;
  RayenProjTile* t = new (std::nothrow) RayenProjTile();
  if (t == nullptr) return nullptr;
  t->L = L;
  t->n = n; t->m = m; t->kg = (n + 7) / 8; t->nx = (n + 31) / 32;
  const int blocks = L.Mp / 32, kg = t->kg, nx = t->nx;
  auto g_at = [&](int prow, int colj) -> float {
    const int row = L.perm[prow];
    return (row >= 0 && colj < n) ? (float)G[(size_t)row * n + colj] : 0.0f;
  };
  // G by row block: [block][g][lane] -> G[32 block + (lane & 31)][8 g + 4 (lane >> 5) + e], e = 0..3
  std::vector<float4> Gi((size_t)blocks * kg * 64), GTi((size_t)blocks * nx * 4 * 64), Ki((size_t)nx * kg * 64);
  for (int b = 0; b < blocks; ++b)
    for (int g = 0; g < kg; ++g)
      for (int l = 0; l < 64; ++l) {
        const int r = 32 * b + (l & 31), c = 8 * g + 4 * (l >> 5);
        Gi[((size_t)b * kg + g) * 64 + l] = make_float4(g_at(r, c), g_at(r, c + 1), g_at(r, c + 2), g_at(r, c + 3));
      }
  // G' by the same blocks: [block][ob][g][lane] -> G[32 block + 8 g + 4 (lane >> 5) + e][32 ob + (lane & 31)]
  for (int b = 0; b < blocks; ++b)
    for (int ob = 0; ob < nx; ++ob)
      for (int g = 0; g < 4; ++g)
        for (int l = 0; l < 64; ++l) {
          const int r = 32 * b + 8 * g + 4 * (l >> 5), c = 32 * ob + (l & 31);
          GTi[(((size_t)b * nx + ob) * 4 + g) * 64 + l] = make_float4(g_at(r, c), g_at(r + 1, c), g_at(r + 2, c), g_at(r + 3, c));
        }
  // Kinv: [ob][g][lane] -> Kinv[k = 8 g + 4 (lane >> 5) + e][32 ob + (lane & 31)]
  auto k_at = [&](int k, int j) -> float { return (k < n && j < n) ? (float)Kinv[(size_t)k * n + j] : 0.0f; };
  for (int ob = 0; ob < nx; ++ob)
    for (int g = 0; g < kg; ++g)
      for (int l = 0; l < 64; ++l) {
        const int k = 8 * g + 4 * (l >> 5), j = 32 * ob + (l & 31);
        Ki[((size_t)ob * kg + g) * 64 + l] = make_float4(k_at(k, j), k_at(k + 1, j), k_at(k + 2, j), k_at(k + 3, j));
      }
  std::vector<float> hi((size_t)L.Mp, 0.0f), wi((size_t)nx * 32, 0.0f);
  for (int r = 0; r < L.Mp; ++r)
    if (L.perm[r] >= 0) hi[r] = (float)h[L.perm[r]];
  for (int j = 0; j < n; ++j) wi[j] = (float)w0[j];
  std::vector<int2> ci(std::max<size_t>(L.cone_rows.size(), 1), make_int2(0, 1));
  for (size_t c = 0; c < L.cone_rows.size(); ++c) ci[c] = make_int2(L.cone_row0[c], L.cone_rows[c]);
  const bool ok = upload_image(Gi, &t->Gimg) && upload_image(GTi, &t->GTimg) && upload_image(Ki, &t->Kimg) &&
                  upload_image(hi, &t->himg) && upload_image(wi, &t->w0img) && upload_image(L.perm, &t->perm) &&
                  upload_image(ci, &t->cones);
  if (!ok) {
    proj_tile_destroy(t);
    return nullptr;
  }
  return t;
}

void proj_tile_destroy(RayenProjTile* t) {
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

int rayen_proj_tile_layout(int32_t m_lin, const int32_t* soc_rows, int32_t n_soc, int32_t* Mp, int32_t* perm_out,
                           int32_t* wave_first_block_out) {
  if (Mp == nullptr || m_lin < 0 || n_soc < 0 || (n_soc > 0 && soc_rows == nullptr)) return RAYEN_E_BAD_ARG;
  for (int c = 0; c < n_soc; ++c)
    if (soc_rows[c] < 1) return RAYEN_E_BAD_ARG;
  Layout L;
  if (n_soc > kMaxCones || !tile_layout(m_lin, soc_rows, n_soc, max_blocks(1), &L)) return RAYEN_E_UNSUPPORTED;
  *Mp = L.Mp;
  if (perm_out != nullptr) std::memcpy(perm_out, L.perm.data(), sizeof(int32_t) * (size_t)L.Mp);
  if (wave_first_block_out != nullptr) std::memcpy(wave_first_block_out, L.first_block, sizeof(L.first_block));
  return RAYEN_OK;
}

int rayen_proj_tile_served(const RayenProjPack* pack) {
  return pack != nullptr && pack->tile != nullptr && pack->psd_dim == 0 && pack->unclaimed == 0;
}

int64_t rayen_proj_tile_workspace_bytes(const RayenProjPack* pack, int64_t B, int32_t backward) {
  (void)backward;                              // (the same regions either way: the backward keeps v*'s data in LDS)
  if (pack == nullptr || B < 0) return -1;
  if (pack->tile == nullptr) return 0;
  return (int64_t)tile_ws(pack->tile, B).total;
}

int rayen_proj_tile_forward_f32(const RayenProjPack* pack, const float* q, int64_t B, int64_t ldq, float* z, int64_t ldz,
                                int32_t* iters, float* vstar, double eps, int32_t max_iters, void* ws, int64_t ws_bytes,
                                void* stream) {
  return run<false>(pack, q, B, ldq, z, ldz, iters, vstar, eps, max_iters, ws, ws_bytes, stream);
}

int rayen_proj_tile_backward_f32(const RayenProjPack* pack, const float* g, int64_t B, int64_t ldg, const float* vstar,
                                 const int32_t* iters, float* grad_q, int64_t ldgq, double eps, int32_t max_iters, void* ws,
                                 int64_t ws_bytes, void* stream) {
  return run<true>(pack, g, B, ldg, grad_q, ldgq, const_cast<int32_t*>(iters), const_cast<float*>(vstar), eps, max_iters,
                   ws, ws_bytes, stream);
}

}  // extern "C"
