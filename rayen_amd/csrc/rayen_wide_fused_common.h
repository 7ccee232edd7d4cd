// What the fused wide forward (rayen_wide_fused.hip) and the fused wide backward (rayen_wide_fused_bwd.hip) share: the
// forward's image of W_ext = [W ; NA_E] (rayen_wide_fused_layout.h), the lock under which the lazy images of a pack are
// built, and the 32 rows x 32 samples product on v_mfma_f32_32x32x2_f32 with its register layout.
#pragma once

#include "rayen_internal.h"
#include "rayen_wide_fused_layout.h"

#include <mutex>
#include <vector>

namespace rayen {

struct FSeg {   // 48 bytes
  int32_t type, row0, nrows, aux_row;
  int32_t first_block, last_block, wave_first, wave_last;
  int32_t part_off, aux_off;
  float f0, f1;
};
struct FItem {  // what a wave does with a block's accumulators: kind 0 = the segment's reduction, 1 / 2 = capture aux row 0 / 1
  int32_t seg, kind;
};

struct WideFusedImage {
  float* W = nullptr;            // [rows_pad][kp]
  float* y0 = nullptr;           // [k]
  FSeg* segs = nullptr;          // [n_seg]
  int32_t* item_start = nullptr; // [nb_w + 1]
  FItem* items = nullptr;
  int n_seg = 0;
  int n_simd = 1024;
  WideFusedPlan plan;
  int64_t bytes = 0;
};

// the lock of a pack's lazy images (wf32 and wfb32): one for the library, taken for the time of a state test or a build
std::mutex& wide_fused_mutex();

// the row-major image of W_ext on the host: [plan.rows_pad][plan.kp], zero in every padded row and column
inline std::vector<float> wide_fused_rows_image(const RayenPack* p, const WideFusedPlan& plan) {
  const int n = p->n, kp = plan.kp;
  std::vector<float> W((size_t)plan.rows_pad * kp, 0.0f);
  for (int r = 0; r < p->n_rows; ++r)
    for (int j = 0; j < n; ++j) W[(size_t)r * kp + j] = (float)p->W[(size_t)r * n + j];
  if (!p->out_identity)
    for (int r = 0; r < p->k; ++r)
      for (int j = 0; j < n; ++j) W[((size_t)plan.rows_w_pad + r) * kp + j] = (float)p->NA_E[(size_t)r * n + j];
  return W;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

// register i of a block's accumulator in half-wave `half`: its row of the block (the lane's column is lane & 31)
__device__ __forceinline__ int row_of(int i, int half) { return 8 * (i >> 2) + 4 * half + (i & 3); }

#define RAYEN_WF_MFMA4(A, Bv, ACC)                                          \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).x, (Bv).x, ACC, 0, 0, 0);  \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).y, (Bv).y, ACC, 0, 0, 0);  \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).z, (Bv).z, ACC, 0, 0, 0);  \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).w, (Bv).w, ACC, 0, 0, 0)

// 32 rows of the image x the tile: `arow` = this lane's row at its half-wave's k offset, `brow` = its sample likewise.
// Chunks of four groups (32 k): the pieces of W of chunk c + 1 are in flight while the MFMAs of chunk c run; what is left
// of K beyond whole chunks (at most three groups) follows one group at a time.  No branch inside a chunk.
__device__ __forceinline__ f32x16 block_product(const float* __restrict__ arow, const float* brow, const int groups) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  const int chunks = groups >> 2;
  if (chunks > 0) {
    float4 a[4], an[4], b[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) a[g] = *reinterpret_cast<const float4*>(arow + 8 * g);
    for (int c = 0; c + 1 < chunks; ++c) {
#pragma unroll
      for (int g = 0; g < 4; ++g) an[g] = *reinterpret_cast<const float4*>(arow + 32 * (c + 1) + 8 * g);
#pragma unroll
      for (int g = 0; g < 4; ++g) b[g] = *reinterpret_cast<const float4*>(brow + 32 * c + 8 * g);
      __builtin_amdgcn_sched_barrier(0);        // (the scheduler otherwise sinks the loads to their use: no prefetch left)
#pragma unroll
      for (int g = 0; g < 4; ++g) { RAYEN_WF_MFMA4(a[g], b[g], acc); }
#pragma unroll
      for (int g = 0; g < 4; ++g) a[g] = an[g];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) b[g] = *reinterpret_cast<const float4*>(brow + 32 * (chunks - 1) + 8 * g);
#pragma unroll
    for (int g = 0; g < 4; ++g) { RAYEN_WF_MFMA4(a[g], b[g], acc); }
  }
  for (int g = 4 * chunks; g < groups; ++g) {
    const float4 a = *reinterpret_cast<const float4*>(arow + 8 * g);
    const float4 b = *reinterpret_cast<const float4*>(brow + 8 * g);
    RAYEN_WF_MFMA4(a, b, acc);
  }
  return acc;
}

}  // namespace rayen
