// Grouping by active constraint for the fused wide backwards (rayen_wide_fused_bwd.hip in fp32, rayen_wide_fused_bwd64.hip in
// fp64): count, scan, scatter over the keys of rayen_wide_fused_bwd_layout.h into the caller's workspace (int32 cursors and
// permutation) -- no allocation, no host synchronisation, any number of segments.  One source for both precisions: T is the
// type of kappa, Seg the segment record of the kernel (any struct with an int32 `key`).  Order inside a bucket is whatever
// the atomics give (no bit of a gradient depends on it).
#pragma once

#include "rayen_internal.h"
#include "rayen_wide_fused_bwd_layout.h"

namespace rayen {

template <typename T, typename Seg>
__device__ __forceinline__ int bwd_key_of(const Seg* __restrict__ segs, const int n_seg, const T kap, const int ag) {
  if (!(kap > (T)1) || ag < 0 || ag >= n_seg) return 0;
  return segs[ag].key;
}

// (both passes over the batch: ONE atomic per wave and distinct key in it -- a batch is a few keys, and an atomic per row
// on so few addresses took longer than the backward itself)
template <typename T, typename Seg>
__global__ __launch_bounds__(256) void bwd_count_kernel(const Seg* __restrict__ segs, int n_seg, const T* __restrict__ kappa,
                                                        const int32_t* __restrict__ active, int64_t B, int32_t* cursors) {
  const int lane = threadIdx.x & 63;
  for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < B; b0 += (int64_t)gridDim.x * 256) {
    const int64_t b = b0 + threadIdx.x;
    const int key = b < B ? bwd_key_of(segs, n_seg, kappa[b], active[2 * b]) : 0;
    unsigned long long todo = __ballot(key > 0);             // (key 0 is what is left: it starts at 0)
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int k0 = __shfl(key, leader, 64);
      const unsigned long long same = __ballot(key == k0);
      if (lane == leader) atomicAdd(cursors + k0, __popcll(same));
      todo &= ~same;
    }
  }
}

// counts -> first positions, by ONE workgroup (rayen_wide_fused_bwd_layout.h::wide_fused_bwd_scan restates it); key 0's count
// is B minus the others'.  (T only keeps the two precisions' instances apart.)
template <typename T>
__global__ __launch_bounds__(256) void bwd_scan_kernel(int32_t* cursors, int64_t n_keys, int64_t B) {
  __shared__ int64_t sums[256];
  const int t = threadIdx.x;
  const int64_t chunk = (n_keys + 255) / 256;
  const int64_t i0 = chunk * t, i1 = (chunk * (t + 1) < n_keys) ? chunk * (t + 1) : n_keys;
  int64_t sum = 0;
  for (int64_t i = i0 > 0 ? i0 : 1; i < i1; ++i) sum += cursors[i];
  sums[t] = sum;
  __syncthreads();
  if (t == 0) {
    int64_t total = 0;
    for (int w = 0; w < 256; ++w) total += sums[w];
    int64_t base = B - total;                              // key 0's count: thread 0's chunk starts behind it
    for (int w = 0; w < 256; ++w) { const int64_t s = sums[w]; sums[w] = base; base += s; }
  }
  __syncthreads();
  int64_t at = sums[t];
  for (int64_t i = i0; i < i1; ++i) {
    if (i == 0) { cursors[0] = 0; continue; }
    const int32_t c = cursors[i];
    cursors[i] = (int32_t)at;
    at += c;
  }
}

template <typename T, typename Seg>
__global__ __launch_bounds__(256) void bwd_scatter_kernel(const Seg* __restrict__ segs, int n_seg, const T* __restrict__ kappa,
                                                          const int32_t* __restrict__ active, int64_t B, int32_t* cursors,
                                                          int32_t* __restrict__ perm) {
  const int lane = threadIdx.x & 63;
  for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < B; b0 += (int64_t)gridDim.x * 256) {
    const int64_t b = b0 + threadIdx.x;
    const int key = b < B ? bwd_key_of(segs, n_seg, kappa[b], active[2 * b]) : -1;
    unsigned long long todo = __ballot(key >= 0);
    int at = -1;
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int k0 = __shfl(key, leader, 64);
      const unsigned long long same = __ballot(key == k0);
      int base = 0;
      if (lane == leader) base = atomicAdd(cursors + k0, __popcll(same));
      base = __shfl(base, leader, 64);
      if (key == k0) at = base + __popcll(same & ((1ull << lane) - 1ull));
      todo &= ~same;
    }
    if (at >= 0 && at < B) perm[at] = (int32_t)b;
  }
}

// The permutation of a batch into `workspace`, where the caller brought room for it (`n_nl` non-linear segments): the three
// launches on `stream`.  *perm: the permutation, null where there is no room (batch order).  False: a launch failed.
template <typename T, typename Seg>
inline bool bwd_group(const Seg* segs, const int n_seg, const int n_nl, const int n_simd, const T* kappa, const int32_t* active,
                      const int64_t B, void* workspace, const int64_t workspace_bytes, hipStream_t stream, const int32_t** perm) {
  *perm = nullptr;
  const int64_t need = wide_fused_bwd_workspace(n_nl, B);
  if (workspace == nullptr || need <= 0 || workspace_bytes < need) return true;
  const int64_t n_keys = (int64_t)n_nl + 1;
  int32_t* cursors = static_cast<int32_t*>(workspace);
  int32_t* pm = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + wide_fused_bwd_perm_offset(n_keys));
  if (hipMemsetAsync(cursors, 0, (size_t)(4 * n_keys), stream) != hipSuccess) return false;
  const int64_t want = (B + 255) / 256, cap = (int64_t)launch_simds(n_simd);
  const unsigned g = (unsigned)(want < cap ? want : cap);
  hipLaunchKernelGGL((bwd_count_kernel<T, Seg>), dim3(g), dim3(256), 0, stream, segs, n_seg, kappa, active, B, cursors);
  hipLaunchKernelGGL((bwd_scan_kernel<T>), dim3(1), dim3(256), 0, stream, cursors, n_keys, B);
  hipLaunchKernelGGL((bwd_scatter_kernel<T, Seg>), dim3(g), dim3(256), 0, stream, segs, n_seg, kappa, active, B, cursors, pm);
  *perm = pm;
  return true;
}

}  // namespace rayen
