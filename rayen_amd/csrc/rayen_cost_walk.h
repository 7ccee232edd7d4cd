// The soft-cost walks over an image of stacked rows in LDS, as functions: what the resident kernels of rayen_cost.hip do
// per tile (fp32) or per item (fp64), with the accumulators passed in, so that the streamed kernels of
// rayen_cost_stream.hip can walk a WINDOW of the image at a time and carry the accumulators from window to window.  A
// sample sees the same operations in the same order on either route, and the two agree bit for bit.
//
// This is a second statement of that arithmetic, not the only one: rayen_cost.hip keeps its kernels as they were written
// (with the walks moved here, hipcc allocated the resident kernels' registers differently -- the fp64 K = 64 instance
// spilled 812 bytes instead of 500, the K = 16 one went from 168 to 202 VGPRs -- and the resident route's timings are a
// bar of the project).  A change to the arithmetic in either file is a change to both; tests/test_gpu_soft_cost_stream.py
// holds the two routes against each other bit for bit.  The image layouts and the lane / register maps are described at
// the top of rayen_cost.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace rayen {
namespace cost {

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { CT_LIN = 0, CT_EQ = 1, CT_QUAD = 2, CT_SOC = 3 };

constexpr int kThreads = 256;                  // four waves: one per SIMD (the image takes most of the CU's LDS)
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

// fp32: the `nt` tiles of an image (W | rowc | colv | desc, all in LDS) against the 32 samples of a wave (yr: this lane's
// half of its sample's y).  Adds to the accumulators: cost_half (this lane half's rows), cost_full (whole-sample terms),
// (wv, wi) the largest value so far and its index, gacc the gradient.  `t` indexes rowc and desc of THIS image; the ids the
// descriptors carry are the set's.
template <bool GRAD>
__device__ __forceinline__ void walk32(const float* __restrict__ W, const float* __restrict__ rowc,
                                       const float* __restrict__ colv, const int* __restrict__ desc, const int nt,
                                       const float (&yr)[32], const int i, const int h, const int eq_shift, f32x16 (&gacc)[2],
                                       float& cost_half, float& cost_full, float& wv, int& wi) {
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
}

// the wave's 32 samples: this lane's half of its sample's row of y (nothing is read for a sample >= B: its y is 0)
__device__ __forceinline__ void load_y32(const float* __restrict__ y, const int64_t s, const bool live, const int64_t ld,
                                         const int k, const int vec_in, const int h, float (&yr)[32]) {
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

// the halves meet, the NaN rule, and the sample's outputs
template <bool GRAD>
__device__ __forceinline__ void store32(const float cost_half, const float cost_full, float wv, int wi, const f32x16 (&gacc)[2],
                                        const int64_t s, const bool live, const int h, const int k, float* __restrict__ cost,
                                        float* __restrict__ worst, int32_t* __restrict__ which, float* __restrict__ grad,
                                        const int64_t ldg, const int vec_out) {
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

// ---- fp64: a lane per sample

template <int K>
__device__ __forceinline__ double dot64(const double* __restrict__ w, const double (&yv)[K]) {
  double a = 0.0;
#pragma unroll
  for (int c = 0; c < K; ++c) a = fma(w[c], yv[c], a);
  return a;
}

// fp64: the `ni` items of an image (W | rowc | colv | fc | desc, all in LDS) against this lane's sample (yv: its y in
// registers, ys: the same row in memory, which the quadratics index).  Adds to cs, (wv, wi) and gv.  Rows are indexed
// within THIS image; the ids are the set's.
template <int K, bool GRAD>
__device__ __forceinline__ void walk64(const double* __restrict__ W, const double* __restrict__ rowc,
                                       const double* __restrict__ colv, const double* __restrict__ fc,
                                       const int* __restrict__ desc, const int ni, const double* __restrict__ ys, const int k,
                                       const double (&yv)[K], const int eq_shift, double (&gv)[K], double& cs, double& wv,
                                       int& wi) {
  for (int it = 0; it < ni; ++it) {
    const int* d = desc + it * kDescWords;
    const int type = d[0], row0 = d[1], id0 = d[2], form = d[3], nrows = d[5];
    const double fconst = fc[it];
    if (type == CT_LIN || type == CT_EQ) {
      const int idr = type == CT_EQ ? id0 + eq_shift : id0;
      for (int r = 0; r < nrows; ++r) {
        const double* __restrict__ w = W + (size_t)(row0 + r) * K;
        const double g = dot64<K>(w, yv) - rowc[row0 + r];
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
      for (int r = 0; r < k; ++r) g = fma(ys[r], fma(0.5, dot64<K>(W + (size_t)(row0 + r) * K, yv), q[r]), g);
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
        const double u = dot64<K>(W + (size_t)(row0 + r) * K, yv) + rowc[row0 + r];
        n2 = fma(u, u, n2);
      }
      const double nrm = sqrt(n2);
      const double g = nrm - dot64<K>(cv, yv) - fconst;
      const double p = relu_(g);
      cs = fma(p, p, cs);
      if (g > wv) { wv = g; wi = id0; }
      if (GRAD && !(p == 0.0)) {
        const double cf = 2.0 * p;
        const double sc = nrm > 0.0 ? cf / nrm : (nrm == 0.0 ? 0.0 : nrm);
        for (int r = 0; r < nrows; ++r) {
          const double* __restrict__ w = W + (size_t)(row0 + r) * K;
          const double cu = sc * (dot64<K>(w, yv) + rowc[row0 + r]);
#pragma unroll
          for (int c = 0; c < K; ++c) gv[c] = fma(cu, w[c], gv[c]);
        }
#pragma unroll
        for (int c = 0; c < K; ++c) gv[c] = fma(-cf, cv[c], gv[c]);
      }
    }
  }
}

}  // namespace cost
}  // namespace rayen
