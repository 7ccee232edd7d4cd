// What the two routes of method='Bar' share (rayen_bar.hip: the image resident in LDS; rayen_bar_stream.hip: the image
// streamed through LDS in windows): the pack, the image's layout, the lane-group geometry, the 16-byte pieces of a row and
// the group reductions.  Both kernels make every lane do the same operations on the same operands in the same order, so
// where both serve a pack their results agree bit for bit (tests/test_gpu_bar_stream.py).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rayen_side_pack.h"

struct RayenBarPack {
  int device = -1, k = 0, nv = 0, nr = 0, K = 0, cus = 0;
  float* img32 = nullptr;     // [round_up(m, 4) + 1][K]
  double* img64 = nullptr;
};

namespace rayen {
namespace bar {

constexpr int kThreads = 512;
constexpr int kMinK = 4, kMaxK = 64;          // the kernels' K: k padded to a power of two between these

__device__ __forceinline__ float exp_(float x) { return expf(x); }
__device__ __forceinline__ double exp_(double x) { return exp(x); }
__device__ __forceinline__ float log_(float x) { return logf(x); }
__device__ __forceinline__ double log_(double x) { return log(x); }

// four consecutive elements of a row: one 16-byte load (fp32) or two (fp64) where the row's pieces are aligned and whole,
// element loads otherwise (a ragged last piece never reads past column m)
template <typename T>
__device__ __forceinline__ void load4(const T* __restrict__ p, bool vec, int left, T (&v)[4]) {
  if (vec && left >= 4) {
    if constexpr (sizeof(T) == 4) {
      const float4 f = *reinterpret_cast<const float4*>(p);
      v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
      const double2 a = reinterpret_cast<const double2*>(p)[0];
      const double2 b = reinterpret_cast<const double2*>(p)[1];
      v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = c < left ? p[c] : T(0);
  }
}

template <typename T>
__device__ __forceinline__ void store4(T* __restrict__ p, bool vec, int left, const T (&v)[4]) {
  if (vec && left >= 4) {
    if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      reinterpret_cast<double2*>(p)[0] = make_double2(v[0], v[1]);
      reinterpret_cast<double2*>(p)[1] = make_double2(v[2], v[3]);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < left) p[c] = v[c];
  }
}

// Where generator j's coefficients sit in the image: within each aligned group of four generators the slot is XORed with
// the group's index mod 4.  The L lanes of a row read generators 4p + c (p = lane, lane + L, ...) at the same c; without
// the swizzle all of them hit the same banks (K = 16: a 256-byte stride), with it four different ones.
__host__ __device__ __forceinline__ int gen_slot(int j) { return (j & ~3) | ((j & 3) ^ ((j >> 2) & 3)); }

template <typename T>
__device__ __forceinline__ T group_sum(T v, int L) {
  for (int off = L >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, L);
  return v;
}

template <typename T>
__device__ __forceinline__ T group_max(T v, int L) {
  for (int off = L >> 1; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, L));
  return v;
}

inline int group_log2(int m) {
  const int pieces = (m + 3) / 4;
  int lg = 0;
  while ((1 << lg) < pieces && lg < 4) ++lg;
  return lg;
}

template <typename T> inline const T* image(const RayenBarPack* p);
template <> inline const float* image<float>(const RayenBarPack* p) { return p->img32; }
template <> inline const double* image<double>(const RayenBarPack* p) { return p->img64; }

// bytes of the image: what the resident kernels keep in LDS
template <typename T>
inline size_t lds_bytes(const RayenBarPack* p) { return (size_t)(((p->nv + p->nr + 3) & ~3) + 1) * p->K * sizeof(T); }

// a leading dimension in 4-byte words: what rayen::rows_aligned16 counts in
template <typename T>
inline int64_t ld_words(int64_t ld) { return ld * (int64_t)(sizeof(T) / 4); }

// rows per launch: every launch's rows span less than 4 GiB of q, y and grad_q (row offsets stay in 32 bits)
inline int64_t rows_per_launch(int64_t ld, size_t elem) {
  const int64_t r = (int64_t)((((uint64_t)1) << 32) / ((uint64_t)(ld > 0 ? ld : 1) * elem));
  return r > 0 ? r : 1;
}

}  // namespace bar
}  // namespace rayen
