// Soft cost and violation of a batch against the ORIGINAL constraints (the reference's examples/cost_computer.py:69-110 and
// the residual metric of ConvexConstraints.getResiduals), loss and gradient in ONE launch:
//
//     cost[b]  = sum_r relu(g_r(y_b))^2 + sum_r (A2 y_b - b2)_r^2        g: A1 y - b1 | 0.5 y'Py + q'y + r | ||My + s|| - c'y - d
//     worst[b] = the largest g_r (with |A2 y - b2|_r counted),  which[b] = its index in the order lin_ineq, quad, soc, lin_eq
//     (a set's LMI, one value between soc and lin_eq, is rayen_cost_lmi.hip's: a second launch that adds to this one's
//     outputs; the kernels here then write the equality rows' indices one higher -- eq_shift, 0 without an LMI)
//     grad[b]  = d cost[b] / d y_b = sum 2 relu(g) a + 2 relu(g) (P y + q) + 2 relu(g) (M'(My + s)/||My + s|| - c) + 2 A2'(A2 y - b2)
//
// fp32: a wave owns 32 samples.  The stacked rows W (A1 | P_i | M_j | A2, padded to tiles of 32 rows x 64 columns) are
// resident in LDS; T = W Y' runs on v_mfma_f32_32x32x2_f32 with the SAMPLE on the lane (column of the result) and 16 of a
// tile's 32 rows in the lane's registers, the other 16 in lane ^ 32, so every per-sample reduction is a sum over registers
// plus one exchange between the halves.  The coefficients C (2 relu(g), 2 relu(g) u / ||u||, 2 e) stay where T was: register
// r of lane half h is row rho(r, h) = (r & 3) + 8 (r >> 2) + 4 h of the tile, which is exactly the k index an MFMA step takes
// from that register, so grad' += W' C' needs no lane movement -- the arrangement of the coefficient step of
// rayen_mfma_bwd.hip.  The same map orders the columns: half h holds columns 4 (2 G + h) + c (G = 0..7, c = 0..3) of its
// sample's y in register 4 G + c and its gradient in the matching accumulator register, so y is read and grad is written in
// 16-byte pieces, and P y of a quadratic (the tile pair itself) lines up with y and with grad register by register: no second
// product for the quadratics.
//
// fp64: a lane per sample over the same image in natural order (LDS, broadcast reads); cones and quadratics take a second
// pass over their rows for the gradient instead of holding the products.
//
// The walks over the image (the bodies of the two kernels' loops over tiles / items) are stated a second time in
// rayen_cost_walk.h for the streamed route (rayen_cost_stream.hip), which must agree with these kernels bit for bit
// (tests/test_gpu_soft_cost_stream.py): a change to the arithmetic here is a change there.
//
// Bounds: a lane whose sample is >= B reads nothing (its y is 0) and writes nothing; columns >= k are never touched in
// y / grad (ld > k is skipped over); every LDS offset comes from the tile table the host built with the image.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "rayen_cost_pack.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { CT_LIN = 0, CT_EQ = 1, CT_QUAD = 2, CT_SOC = 3 };

constexpr int kThreads = 256;                  // four waves: one per SIMD (the image takes most of the CU's LDS)
using rayen::kLdsBudget;
constexpr int kMinK64 = 8, kMaxK64 = 64;       // the fp64 kernel's K: k padded to a power of two between these
constexpr int kDescWords = 8;                  // per tile / item: type, nvalid | row0, id0, form, fconst, ntiles | nrows, -, -

// row of a 32-row tile that register r of lane half h holds (C/D map of the 32x32 MFMA), also the k index of MFMA step r
__host__ __device__ __forceinline__ int rho(const int r, const int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// where the 16-byte piece p of tile row R sits in the row (16 pieces): XOR with the row keeps the 16 lanes of a ds_read_b128
// group (16 different rows, the same piece) on 16 different slots, and the 32 lanes of a ds_read_b32 of one row on 32 banks
__host__ __device__ __forceinline__ int piece_slot(const int p, const int R) { return p ^ (R & 15); }

__device__ __forceinline__ float other_half(const float v) { return __shfl_xor(v, 32, 64); }
__device__ __forceinline__ int other_half(const int v) { return __shfl_xor(v, 32, 64); }

// relu that keeps a NaN (fmaxf would answer 0)
template <typename T>
__device__ __forceinline__ T relu_(const T g) { return g < T(0) ? T(0) : g; }

// T tile = W[tile rows] Y': acc register r = row rho(r, h) of the tile, for this lane's sample
__device__ __forceinline__ f32x16 tile_product(const float* __restrict__ Wt, const float (&yr)[32], const int i, const int h) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const float4* __restrict__ row = reinterpret_cast<const float4*>(Wt + i * 64);
#pragma unroll
  for (int G = 0; G < 8; ++G) {
    const float4 a = row[piece_slot(2 * G + h, i)];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, yr[4 * G + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, yr[4 * G + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, yr[4 * G + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, yr[4 * G + 3], acc, 0, 0, 0);
  }
  return acc;
}

// gacc[tp] register r' (column rho(r', h) + 32 tp of grad) += sum over the tile's rows of C[sample][row] W[row][column]
__device__ __forceinline__ void coef_product(const float* __restrict__ Wt, const f32x16& cf, f32x16 (&gacc)[2], const int i,
                                             const int h) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int R = rho(r, h);
    const float* __restrict__ row = Wt + R * 64 + (i & 3);
#pragma unroll
    for (int tp = 0; tp < 2; ++tp) {
      const float a = row[piece_slot(8 * tp + (i >> 2), R) * 4];
      gacc[tp] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, cf[r], gacc[tp], 0, 0, 0);
    }
  }
}

template <bool GRAD>
__global__ __launch_bounds__(kThreads) void cost_mfma_kernel(const uint4* __restrict__ img, const int n16, const int nt,
                                                             const int rowc_off, const int colv_off, const int desc_off,
                                                             const float* __restrict__ y, const int64_t B, const int64_t ld,
                                                             const int k, const int vec_in, float* __restrict__ cost,
                                                             float* __restrict__ worst, int32_t* __restrict__ which,
                                                             float* __restrict__ grad, const int64_t ldg, const int vec_out,
                                                             const int eq_shift) {
  extern __shared__ __align__(16) unsigned char cost_smem[];
  {
    uint4* dst = reinterpret_cast<uint4*>(cost_smem);
    for (int p = threadIdx.x; p < n16; p += kThreads) dst[p] = img[p];
    __syncthreads();
  }
  const float* __restrict__ W = reinterpret_cast<const float*>(cost_smem);
  const float* __restrict__ rowc = W + rowc_off;
  const float* __restrict__ colv = W + colv_off;
  const int* __restrict__ desc = reinterpret_cast<const int*>(cost_smem) + desc_off;

  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const int64_t wave = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * (kThreads / 64);
  const int64_t n_groups = (B + 31) / 32;
  const float ninf = -INFINITY;

  for (int64_t grp = wave; grp < n_groups; grp += n_waves) {
    const int64_t s = grp * 32 + i;
    const bool live = s < B;
    float yr[32];
    {
      const float* __restrict__ ys = y + (live ? s : 0) * ld;
#pragma unroll
      for (int G = 0; G < 8; ++G) {
        const int c0 = 4 * (2 * G + h);
        if (vec_in && live && c0 + 4 <= k) {
          const float4 f = *reinterpret_cast<const float4*>(ys + c0);
          yr[4 * G + 0] = f.x; yr[4 * G + 1] = f.y; yr[4 * G + 2] = f.z; yr[4 * G + 3] = f.w;
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) yr[4 * G + c] = (live && c0 + c < k) ? ys[c0 + c] : 0.0f;
        }
      }
    }
    f32x16 gacc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[0][r] = gacc[1][r] = 0.0f;
    float cost_half = 0.0f, cost_full = 0.0f, wv = ninf;     // cost_half: this lane half's rows | cost_full: whole-sample terms
    int wi = -1;

    int t = 0;
    while (t < nt) {
      const int* d = desc + t * kDescWords;
      const int type = __builtin_amdgcn_readfirstlane(d[0]);
      const int nvalid = __builtin_amdgcn_readfirstlane(d[1]);
      const int id0 = __builtin_amdgcn_readfirstlane(d[2]);
      const int form = __builtin_amdgcn_readfirstlane(d[3]);
      const float fconst = __int_as_float(__builtin_amdgcn_readfirstlane(d[4]));
      const int ntile = __builtin_amdgcn_readfirstlane(d[5]);
      const float* __restrict__ Wt = W + (size_t)t * 2048;
      if (type == CT_LIN || type == CT_EQ) {
        f32x16 T0 = tile_product(Wt, yr, i, h);
        const int idr = type == CT_EQ ? id0 + eq_shift : id0;     // (an LMI sits between the inequalities and these)
        bool any = false;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int R = rho(r, h);
          const bool valid = R < nvalid;
          const float g = T0[r] - rowc[t * 32 + R];
          const float p = type == CT_EQ ? g : relu_(g);
          const float val = type == CT_EQ ? fabsf(g) : g;
          if (valid) {
            cost_half = fmaf(p, p, cost_half);
            if (val > wv) { wv = val; wi = idr + R; }
          }
          const float cf = valid ? 2.0f * p : 0.0f;
          T0[r] = cf;
          any |= !(cf == 0.0f);
        }
        if (GRAD && __builtin_amdgcn_ballot_w64(any) != 0) coef_product(Wt, T0, gacc, i, h);
        t += 1;
      } else if (type == CT_QUAD) {
        const f32x16 T0 = tile_product(Wt, yr, i, h);
        const f32x16 T1 = tile_product(Wt + 2048, yr, i, h);
        const float* __restrict__ q = colv + form * 64;
        float part = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int R = rho(r, h);
          part = fmaf(yr[r], fmaf(0.5f, T0[r], q[R]), part);
          part = fmaf(yr[16 + r], fmaf(0.5f, T1[r], q[32 + R]), part);
        }
        const float g = part + other_half(part) + fconst;
        const float p = relu_(g);
        cost_full = fmaf(p, p, cost_full);
        if (g > wv) { wv = g; wi = id0; }
        if (GRAD && !(p == 0.0f)) {
          const float c2 = 2.0f * p;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int R = rho(r, h);
            gacc[0][r] = fmaf(c2, T0[r] + q[R], gacc[0][r]);
            gacc[1][r] = fmaf(c2, T1[r] + q[32 + R], gacc[1][r]);
          }
        }
        t += 2;
      } else {  // CT_SOC: one or two tiles of M rows
        f32x16 T0 = tile_product(Wt, yr, i, h);
        f32x16 T1;
        if (ntile == 2) {
          T1 = tile_product(Wt + 2048, yr, i, h);
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) T1[r] = 0.0f;
        }
        const float* __restrict__ cv = colv + form * 64;
        float n2 = 0.0f, cy = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int R = rho(r, h);
          const float u0 = R < nvalid ? T0[r] + rowc[t * 32 + R] : 0.0f;
          const float u1 = (ntile == 2 && 32 + R < nvalid) ? T1[r] + rowc[t * 32 + 32 + R] : 0.0f;
          T0[r] = u0;
          T1[r] = u1;
          n2 = fmaf(u0, u0, n2);
          n2 = fmaf(u1, u1, n2);
          cy = fmaf(yr[r], cv[R], cy);
          cy = fmaf(yr[16 + r], cv[32 + R], cy);
        }
        n2 += other_half(n2);
        cy += other_half(cy);
        const float nrm = sqrtf(n2);
        const float g = nrm - cy - fconst;
        const float p = relu_(g);
        cost_full = fmaf(p, p, cost_full);
        if (g > wv) { wv = g; wi = id0; }
        if (GRAD && __builtin_amdgcn_ballot_w64(!(p == 0.0f)) != 0) {
          const float c2 = 2.0f * p;
          const float sc = nrm > 0.0f ? c2 / nrm : (nrm == 0.0f ? 0.0f : nrm);     // (a NaN norm stays a NaN)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int R = rho(r, h);
            T0[r] *= sc;
            T1[r] *= sc;
            gacc[0][r] = fmaf(-c2, cv[R], gacc[0][r]);
            gacc[1][r] = fmaf(-c2, cv[32 + R], gacc[1][r]);
          }
          coef_product(Wt, T0, gacc, i, h);
          if (ntile == 2) coef_product(Wt + 2048, T1, gacc, i, h);
        }
        t += ntile;
      }
    }

    float c = cost_half + other_half(cost_half) + cost_full;
    {
      const float ov = other_half(wv);
      const int oi = other_half(wi);
      if (ov > wv || (ov == wv && oi >= 0 && (wi < 0 || oi < wi))) { wv = ov; wi = oi; }
    }
    if (c != c) { wv = c; wi = -1; }
    if (live && h == 0) {
      if (cost != nullptr) cost[s] = c;
      if (worst != nullptr) worst[s] = wv;
      if (which != nullptr) which[s] = wi;
    }
    if (GRAD && live) {
      float* __restrict__ gs = grad + s * ldg;
#pragma unroll
      for (int G = 0; G < 8; ++G) {
        const int c0 = 4 * (2 * G + h), tp = G >> 2, r0 = 4 * (G & 3);
        if (vec_out && c0 + 4 <= k) {
          *reinterpret_cast<float4*>(gs + c0) = make_float4(gacc[tp][r0], gacc[tp][r0 + 1], gacc[tp][r0 + 2], gacc[tp][r0 + 3]);
        } else {
#pragma unroll
          for (int cc = 0; cc < 4; ++cc)
            if (c0 + cc < k) gs[c0 + cc] = gacc[tp][r0 + cc];
        }
      }
    }
  }
}

// ---- fp64: a lane per sample
template <int K, bool GRAD>
__global__ __launch_bounds__(kThreads) void cost_lane64_kernel(const uint4* __restrict__ img, const int n16, const int ni,
                                                               const int rowc_off, const int colv_off, const int fc_off,
                                                               const int desc_off, const double* __restrict__ y,
                                                               const int64_t B, const int64_t ld, const int k,
                                                               double* __restrict__ cost, double* __restrict__ worst,
                                                               int32_t* __restrict__ which, double* __restrict__ grad,
                                                               const int64_t ldg, const int eq_shift) {
  extern __shared__ __align__(16) unsigned char cost_smem[];
  {
    uint4* dst = reinterpret_cast<uint4*>(cost_smem);
    for (int p = threadIdx.x; p < n16; p += kThreads) dst[p] = img[p];
    __syncthreads();
  }
  const double* __restrict__ W = reinterpret_cast<const double*>(cost_smem);
  const double* __restrict__ rowc = W + rowc_off;
  const double* __restrict__ colv = W + colv_off;
  const double* __restrict__ fc = W + fc_off;
  const int* __restrict__ desc = reinterpret_cast<const int*>(W + desc_off);

  for (int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x; s < B; s += (int64_t)gridDim.x * kThreads) {
    const double* __restrict__ ys = y + s * ld;
    double yv[K], gv[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
      yv[c] = c < k ? ys[c] : 0.0;
      gv[c] = 0.0;
    }
    auto dot = [&](const double* __restrict__ w) {
      double a = 0.0;
#pragma unroll
      for (int c = 0; c < K; ++c) a = fma(w[c], yv[c], a);
      return a;
    };
    double cs = 0.0, wv = -INFINITY;
    int wi = -1;
    for (int it = 0; it < ni; ++it) {
      const int* d = desc + it * kDescWords;
      const int type = d[0], row0 = d[1], id0 = d[2], form = d[3], nrows = d[5];
      const double fconst = fc[it];
      if (type == CT_LIN || type == CT_EQ) {
        const int idr = type == CT_EQ ? id0 + eq_shift : id0;
        for (int r = 0; r < nrows; ++r) {
          const double* __restrict__ w = W + (size_t)(row0 + r) * K;
          const double g = dot(w) - rowc[row0 + r];
          const double p = type == CT_EQ ? g : relu_(g);
          const double val = type == CT_EQ ? fabs(g) : g;
          cs = fma(p, p, cs);
          if (val > wv) { wv = val; wi = idr + r; }
          if (GRAD && !(p == 0.0)) {
            const double cf = 2.0 * p;
#pragma unroll
            for (int c = 0; c < K; ++c) gv[c] = fma(cf, w[c], gv[c]);
          }
        }
      } else if (type == CT_QUAD) {       // rows of the symmetrised P: (P y)_c = sum_r y_r P[r][c]
        const double* __restrict__ q = colv + (size_t)form * K;
        double g = fconst;
        for (int r = 0; r < k; ++r) g = fma(ys[r], fma(0.5, dot(W + (size_t)(row0 + r) * K), q[r]), g);
        const double p = relu_(g);
        cs = fma(p, p, cs);
        if (g > wv) { wv = g; wi = id0; }
        if (GRAD && !(p == 0.0)) {
          const double cf = 2.0 * p;
          for (int r = 0; r < k; ++r) {
            const double* __restrict__ w = W + (size_t)(row0 + r) * K;
            const double cy = cf * ys[r];
#pragma unroll
            for (int c = 0; c < K; ++c) gv[c] = fma(cy, w[c], gv[c]);
          }
#pragma unroll
          for (int c = 0; c < K; ++c) gv[c] = fma(cf, q[c], gv[c]);
        }
      } else {
        const double* __restrict__ cv = colv + (size_t)form * K;
        double n2 = 0.0;
        for (int r = 0; r < nrows; ++r) {
          const double u = dot(W + (size_t)(row0 + r) * K) + rowc[row0 + r];
          n2 = fma(u, u, n2);
        }
        const double nrm = sqrt(n2);
        const double g = nrm - dot(cv) - fconst;
        const double p = relu_(g);
        cs = fma(p, p, cs);
        if (g > wv) { wv = g; wi = id0; }
        if (GRAD && !(p == 0.0)) {
          const double cf = 2.0 * p;
          const double sc = nrm > 0.0 ? cf / nrm : (nrm == 0.0 ? 0.0 : nrm);
          for (int r = 0; r < nrows; ++r) {
            const double* __restrict__ w = W + (size_t)(row0 + r) * K;
            const double cu = sc * (dot(w) + rowc[row0 + r]);
#pragma unroll
            for (int c = 0; c < K; ++c) gv[c] = fma(cu, w[c], gv[c]);
          }
#pragma unroll
          for (int c = 0; c < K; ++c) gv[c] = fma(-cf, cv[c], gv[c]);
        }
      }
    }
    if (cs != cs) { wv = cs; wi = -1; }
    if (cost != nullptr) cost[s] = cs;
    if (worst != nullptr) worst[s] = wv;
    if (which != nullptr) which[s] = wi;
    if (GRAD) {
      double* __restrict__ gs = grad + s * ldg;
#pragma unroll
      for (int c = 0; c < K; ++c)
        if (c < k) gs[c] = gv[c];
    }
  }
}

// ---- host: the images
using SetView = rayen::CostSetView;

int float_bits(const float f) {
  int b;
  std::memcpy(&b, &f, 4);
  return b;
}

}  // namespace

// fp32 image: tiles of 32 rows x 64 columns, 16-byte pieces XORed with the row (piece_slot)
bool rayen::cost_build32(const SetView& v, RayenCostPack* p, std::vector<int32_t>* words, const size_t budget) {
  for (int j = 0; j < v.nsoc; ++j)
    if (v.soc_rows[j] > 64) return false;          // a cone's products are held in two tiles
  const int tl = (v.m1 + 31) / 32, te = (v.m2 + 31) / 32;
  int tsoc = 0;
  for (int j = 0; j < v.nsoc; ++j) tsoc += v.soc_rows[j] > 32 ? 2 : 1;
  const int nt = tl + 2 * v.nq + tsoc + te, nf = v.nq + v.nsoc;
  const size_t n_words = (size_t)nt * 2048 + (size_t)nt * 32 + (size_t)nf * 64 + (size_t)nt * kDescWords;
  const size_t bytes = (n_words * 4 + 15) & ~(size_t)15;
  p->bytes32 = bytes;
  if (bytes > budget) return false;
  p->nt = nt;
  p->rowc_off = nt * 2048;
  p->colv_off = p->rowc_off + nt * 32;
  p->desc_off = p->colv_off + nf * 64;
  std::vector<float> f(bytes / 4, 0.0f);
  std::vector<int32_t>& w = *words;
  w.assign(bytes / 4, 0);
  auto put_row = [&](const int t, const int R, const double* src) {
    for (int c = 0; c < v.k; ++c) f[(size_t)t * 2048 + R * 64 + piece_slot(c >> 2, R) * 4 + (c & 3)] = (float)src[c];
  };
  auto put_desc = [&](const int t, const int type, const int nvalid, const int id0, const int form, const float fconst,
                      const int ntile) {
    int32_t* d = w.data() + p->desc_off + t * kDescWords;
    d[0] = type; d[1] = nvalid; d[2] = id0; d[3] = form; d[4] = float_bits(fconst); d[5] = ntile;
  };
  int t = 0;
  auto linear = [&](const double* A, const double* b, const int m, const int type, const int id_base) {
    for (int r0 = 0; r0 < m; r0 += 32, ++t) {
      const int n = m - r0 < 32 ? m - r0 : 32;
      for (int R = 0; R < n; ++R) {
        put_row(t, R, A + (size_t)(r0 + R) * v.k);
        f[p->rowc_off + t * 32 + R] = (float)b[r0 + R];
      }
      put_desc(t, type, n, id_base + r0, 0, 0.0f, 1);
    }
  };
  linear(v.A1, v.b1, v.m1, CT_LIN, 0);
  for (int iq = 0; iq < v.nq; ++iq, t += 2) {
    const double* P = v.P + (size_t)iq * v.k * v.k;
    std::vector<double> row(v.k);
    for (int r = 0; r < v.k; ++r) {
      for (int c = 0; c < v.k; ++c) row[c] = 0.5 * (P[(size_t)r * v.k + c] + P[(size_t)c * v.k + r]);
      put_row(t + (r >> 5), r & 31, row.data());
      f[p->colv_off + iq * 64 + r] = (float)v.q[(size_t)iq * v.k + r];
    }
    put_desc(t, CT_QUAD, v.k, v.m1 + iq, iq, (float)v.r[iq], 2);
    put_desc(t + 1, CT_QUAD, v.k, v.m1 + iq, iq, (float)v.r[iq], 2);
  }
  size_t mrow = 0;
  for (int j = 0; j < v.nsoc; ++j) {
    const int rows = v.soc_rows[j], ntile = rows > 32 ? 2 : 1;
    for (int r = 0; r < rows; ++r) {
      put_row(t + (r >> 5), r & 31, v.M + (mrow + r) * v.k);
      f[p->rowc_off + t * 32 + r] = (float)v.s[mrow + r];
    }
    for (int c = 0; c < v.k; ++c) f[p->colv_off + (v.nq + j) * 64 + c] = (float)v.c[(size_t)j * v.k + c];
    for (int e = 0; e < ntile; ++e) put_desc(t + e, CT_SOC, rows, v.m1 + v.nq + j, v.nq + j, (float)v.d[j], ntile);
    mrow += rows;
    t += ntile;
  }
  linear(v.A2, v.b2, v.m2, CT_EQ, v.m1 + v.nq + v.nsoc);
  for (size_t e = 0; e < (size_t)p->desc_off; ++e) w[e] = float_bits(f[e]);
  return t == nt;
}

bool rayen::cost_build64(const SetView& v, RayenCostPack* p, std::vector<double>* words, const size_t budget) {
  const int K = rayen::padded_width<kMinK64, kMaxK64>(v.k);
  int64_t msoc = 0;
  for (int j = 0; j < v.nsoc; ++j) msoc += v.soc_rows[j];
  const int64_t R64 = (int64_t)v.m1 + (int64_t)v.nq * v.k + msoc + v.m2;
  const int nf = v.nq + v.nsoc;
  const int ni = (v.m1 > 0) + v.nq + v.nsoc + (v.m2 > 0);
  const size_t n_words = (size_t)R64 * K + (size_t)R64 + (size_t)nf * K + (size_t)ni + (size_t)ni * kDescWords / 2;
  const size_t bytes = (n_words * 8 + 15) & ~(size_t)15;
  p->K64 = K;
  p->ni = ni;
  p->bytes64 = bytes;
  if (bytes > budget) return false;
  const int R = (int)R64;
  p->rowc64_off = R * K;
  p->colv64_off = p->rowc64_off + R;
  p->fc64_off = p->colv64_off + nf * K;
  p->desc64_off = p->fc64_off + ni;
  std::vector<double>& w = *words;
  w.assign(bytes / 8, 0.0);
  int32_t* desc = reinterpret_cast<int32_t*>(w.data() + p->desc64_off);
  int row = 0, it = 0;
  auto put_desc = [&](const int type, const int row0, const int id0, const int form, const double fconst, const int nrows) {
    int32_t* d = desc + it * kDescWords;
    d[0] = type; d[1] = row0; d[2] = id0; d[3] = form; d[5] = nrows;
    w[p->fc64_off + it] = fconst;
    ++it;
  };
  auto linear = [&](const double* A, const double* b, const int m, const int type, const int id_base) {
    if (m <= 0) return;
    put_desc(type, row, id_base, 0, 0.0, m);
    for (int r = 0; r < m; ++r, ++row) {
      for (int c = 0; c < v.k; ++c) w[(size_t)row * K + c] = A[(size_t)r * v.k + c];
      w[p->rowc64_off + row] = b[r];
    }
  };
  linear(v.A1, v.b1, v.m1, CT_LIN, 0);
  for (int iq = 0; iq < v.nq; ++iq) {
    const double* P = v.P + (size_t)iq * v.k * v.k;
    put_desc(CT_QUAD, row, v.m1 + iq, iq, v.r[iq], v.k);
    for (int r = 0; r < v.k; ++r, ++row) {
      for (int c = 0; c < v.k; ++c) w[(size_t)row * K + c] = 0.5 * (P[(size_t)r * v.k + c] + P[(size_t)c * v.k + r]);
      w[p->colv64_off + (size_t)iq * K + r] = v.q[(size_t)iq * v.k + r];
    }
  }
  size_t mrow = 0;
  for (int j = 0; j < v.nsoc; ++j) {
    put_desc(CT_SOC, row, v.m1 + v.nq + j, v.nq + j, v.d[j], v.soc_rows[j]);
    for (int r = 0; r < v.soc_rows[j]; ++r, ++row, ++mrow) {
      for (int c = 0; c < v.k; ++c) w[(size_t)row * K + c] = v.M[mrow * v.k + c];
      w[p->rowc64_off + row] = v.s[mrow];
    }
    for (int c = 0; c < v.k; ++c) w[p->colv64_off + (size_t)(v.nq + j) * K + c] = v.c[(size_t)j * v.k + c];
  }
  linear(v.A2, v.b2, v.m2, CT_EQ, v.m1 + v.nq + v.nsoc);
  return row == R && it == ni;
}

namespace {

template <bool GRAD>
int launch32(const RayenCostPack* p, const float* y, int64_t B, int64_t ld, float* cost, float* worst, int32_t* which,
             float* grad, int64_t ldg, hipStream_t stream) {
  auto kern = cost_mfma_kernel<GRAD>;
  if (!rayen::allow_lds(kern, p->bytes32)) return RAYEN_E_LAUNCH;
  const int64_t grid = rayen::persistent_grid(B, 32, rayen::launch_simds(p->n_simd), kThreads / 64);
  const int vec_in = (p->k % 4 == 0) && rayen::rows_aligned16(y, ld);
  const int vec_out = GRAD && (p->k % 4 == 0) && rayen::rows_aligned16(grad, ldg);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kThreads), p->bytes32, stream, reinterpret_cast<const uint4*>(p->img32),
                     (int)(p->bytes32 / 16), p->nt, p->rowc_off, p->colv_off, p->desc_off, y, B, ld, p->k, vec_in, cost,
                     worst, which, grad, ldg, vec_out, p->eq_shift);
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

template <int K, bool GRAD>
int launch64(const RayenCostPack* p, const double* y, int64_t B, int64_t ld, double* cost, double* worst, int32_t* which,
             double* grad, int64_t ldg, hipStream_t stream) {
  auto kern = cost_lane64_kernel<K, GRAD>;
  if (!rayen::allow_lds(kern, p->bytes64)) return RAYEN_E_LAUNCH;
  const int64_t grid = rayen::persistent_grid(B, kThreads, rayen::launch_simds(p->n_simd) / 4, 1);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kThreads), p->bytes64, stream, reinterpret_cast<const uint4*>(p->img64),
                     (int)(p->bytes64 / 16), p->ni, p->rowc64_off, p->colv64_off, p->fc64_off, p->desc64_off, y, B, ld,
                     p->k, cost, worst, which, grad, ldg, p->eq_shift);
  return hipGetLastError() == hipSuccess ? RAYEN_OK : RAYEN_E_LAUNCH;
}

template <int K>
int launch64_k(const RayenCostPack* p, const double* y, int64_t B, int64_t ld, double* cost, double* worst, int32_t* which,
               double* grad, int64_t ldg, hipStream_t stream) {
  return grad != nullptr ? launch64<K, true>(p, y, B, ld, cost, worst, which, grad, ldg, stream)
                         : launch64<K, false>(p, y, B, ld, cost, worst, which, grad, ldg, stream);
}

}  // namespace

extern "C" {

int rayen_cost_pack_create(const double* A1, const double* b1, int32_t m1, const double* P, const double* q, const double* r,
                           int32_t nq, const double* M, const double* s, const double* c, const double* d,
                           const int32_t* soc_rows, int32_t nsoc, const double* A2, const double* b2, int32_t m2, int32_t k,
                           RayenCostPack** out) {
  if (out == nullptr) return RAYEN_E_BAD_ARG;
  *out = nullptr;
  if (k <= 0 || m1 < 0 || nq < 0 || nsoc < 0 || m2 < 0) return RAYEN_E_BAD_ARG;     // (no rows: a set that is one LMI)
  if ((m1 > 0 && (A1 == nullptr || b1 == nullptr)) || (nq > 0 && (P == nullptr || q == nullptr || r == nullptr)) ||
      (nsoc > 0 && (M == nullptr || s == nullptr || c == nullptr || d == nullptr || soc_rows == nullptr)) ||
      (m2 > 0 && (A2 == nullptr || b2 == nullptr)))
    return RAYEN_E_BAD_ARG;
  for (int j = 0; j < nsoc; ++j)
    if (soc_rows[j] <= 0) return RAYEN_E_BAD_ARG;
  int dev = -1, cus = 0;
  if (rayen::side_pack_device(&dev, &cus, 256) != RAYEN_OK) return RAYEN_E_NO_DEVICE;
  RayenCostPack* p = new (std::nothrow) RayenCostPack();
  if (p == nullptr) return RAYEN_E_ALLOC;
  p->device = dev;
  p->k = k;
  p->n_simd = cus * 4;
  p->n_rows = m1 + nq + nsoc + m2;
  p->lmi_id = m1 + nq + nsoc;
  if (k <= 64 && p->n_rows > 0) {     // k beyond: the pack exists and a call on its rows answers RAYEN_E_UNSUPPORTED
    // the arrays, kept on the host in this order for the streamed route (rayen_cost_stream.hip: cost_stream_view)
    const size_t kk = (size_t)k;
    size_t msoc = 0;
    for (int j = 0; j < nsoc; ++j) msoc += (size_t)soc_rows[j];
    const double* src[11] = {A1, b1, P, q, r, M, s, c, d, A2, b2};
    const size_t len[11] = {m1 * kk, (size_t)m1, nq * kk * kk, nq * kk, (size_t)nq, msoc * kk, msoc, nsoc * kk, (size_t)nsoc,
                            m2 * kk, (size_t)m2};
    try {
      for (int a = 0; a < 11; ++a) p->host.insert(p->host.end(), src[a], src[a] + len[a]);
      p->host_soc_rows.assign(soc_rows, soc_rows + nsoc);
    } catch (const std::bad_alloc&) {
      delete p;
      return RAYEN_E_ALLOC;
    }
    p->m1 = m1; p->nq = nq; p->nsoc = nsoc; p->m2 = m2;
    const SetView v{A1, b1, P, q, r, M, s, c, d, A2, b2, soc_rows, m1, nq, nsoc, m2, k};
    std::vector<int32_t> w32;
    std::vector<double> w64;
    p->served32 = rayen::cost_build32(v, p, &w32, kLdsBudget);
    p->served64 = rayen::cost_build64(v, p, &w64, kLdsBudget);
    if ((p->served32 && !rayen::upload_image(w32, &p->img32)) || (p->served64 && !rayen::upload_image(w64, &p->img64))) {
      rayen_cost_pack_destroy(p);
      return RAYEN_E_ALLOC;
    }
  }
  *out = p;
  return RAYEN_OK;
}

void rayen_cost_pack_destroy(RayenCostPack* p) {
  if (p == nullptr) return;
  {
    rayen::DeviceScope on_device(p->device);
    if (p->img32) (void)hipFree(p->img32);
    if (p->img64) (void)hipFree(p->img64);
    rayen::cost_lmi_free(p->lmi);
    rayen::cost_stream_free(p->stream);
    rayen::cost_tile64_free(p->tile64);
  }
  delete p;
}

int rayen_cost_pack_set_lmi(RayenCostPack* pack, const double* F, int32_t r) {
  if (pack == nullptr || F == nullptr || r < 1 || pack->lmi != nullptr) return RAYEN_E_BAD_ARG;
  int rc = rayen::check_device(pack->device);
  if (rc != RAYEN_OK) return rc;
  rc = rayen::cost_lmi_build(F, r, pack->k, &pack->lmi);
  if (rc == RAYEN_OK) pack->eq_shift = 1;
  return rc;
}

}  // extern "C"

namespace {

// (the resident route serves the rows whose whole image fits LDS)
template <typename T>
bool serves_set(const RayenCostPack* p) {
  return rayen::cost_serves_set<T>(p, sizeof(T) == 8 ? p->served64 : p->served32);
}

template <typename T, typename Rows>
int soft_cost(const RayenCostPack* pack, const T* y, int64_t B, int64_t ld, T* cost, T* worst, int32_t* which, T* grad,
              int64_t ld_grad, void* stream, Rows&& launch_rows) {
  return rayen::cost_call<T>(pack, pack != nullptr && (sizeof(T) == 8 ? pack->served64 : pack->served32), y, B, ld, cost,
                             worst, which, grad, ld_grad, stream, launch_rows);
}

}  // namespace

extern "C" {

int rayen_cost_served(const RayenCostPack* pack, int32_t f64) {
  if (pack == nullptr) return 0;
  return (f64 ? serves_set<double>(pack) : serves_set<float>(pack)) ? 1 : 0;
}

int rayen_soft_cost_f32(const RayenCostPack* pack, const float* y, int64_t B, int64_t ld, float* cost, float* worst,
                        int32_t* which, float* grad, int64_t ld_grad, void* stream) {
  return soft_cost<float>(pack, y, B, ld, cost, worst, which, grad, ld_grad, stream, [&](hipStream_t st) {
    return grad != nullptr ? launch32<true>(pack, y, B, ld, cost, worst, which, grad, ld_grad, st)
                           : launch32<false>(pack, y, B, ld, cost, worst, which, grad, ld_grad, st);
  });
}

int rayen_soft_cost_f64(const RayenCostPack* pack, const double* y, int64_t B, int64_t ld, double* cost, double* worst,
                        int32_t* which, double* grad, int64_t ld_grad, void* stream) {
  return soft_cost<double>(pack, y, B, ld, cost, worst, which, grad, ld_grad, stream, [&](hipStream_t st) {
    return rayen::dispatch_width<kMinK64, kMaxK64>(pack->K64, [&](auto K) {
      return launch64_k<K()>(pack, y, B, ld, cost, worst, which, grad, ld_grad, st);
    });
  });
}

}  // extern "C"
