// What the fp64 fused wide forward (rayen_wide_fused64.hip) and the fp64 fused wide backward (rayen_wide_fused_bwd64.hip)
// share: the forward's image of W_ext = [W ; NA_E] (rayen_wide_fused64_layout.h) and the 16 rows x NC column blocks product
// on v_mfma_f64_16x16x4_f64 with its two accumulator chains.  The lock of the lazy images is rayen_wide_fused_common.h's.
#pragma once

#include "rayen_internal.h"
#include "rayen_wide_fused64_layout.h"
#include "rayen_wide_fused_common.h"

namespace rayen {

struct F64Seg {   // 56 bytes
  int32_t type, row0, nrows, aux_row;
  int32_t first_block, last_block, wave_first, wave_last;
  int32_t part_off, aux_off;
  double f0, f1;
};

struct WideFused64Image {
  double* W = nullptr;            // [rows_pad][kp]
  double* y0 = nullptr;           // [k]
  F64Seg* segs[2] = {nullptr, nullptr};      // [n_seg], scratch offsets of S = 16 | 32
  int32_t* item_start = nullptr;  // [nb_w + 1]
  FItem* items = nullptr;
  int n_seg = 0;
  int n_simd = 1024;
  WideFused64Plan plan[2];        // S = 16 | 32
  int64_t bytes = 0;
};

// the row-major image of W_ext on the host: [rows_pad][kp] (the rows of NA_E from rows_w_pad), zero in every padded row and
// column
inline std::vector<double> wide_fused64_rows_image(const RayenPack* p, const int rows_w_pad, const int rows_pad, const int kp) {
  const int n = p->n;
  std::vector<double> W((size_t)rows_pad * kp, 0.0);
  for (int r = 0; r < p->n_rows; ++r)
    for (int j = 0; j < n; ++j) W[(size_t)r * kp + j] = p->W[(size_t)r * n + j];
  if (!p->out_identity)
    for (int r = 0; r < p->k; ++r)
      for (int j = 0; j < n; ++j) W[((size_t)rows_w_pad + r) * kp + j] = p->NA_E[(size_t)r * n + j];
  return W;
}

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

#define RAYEN_WF64_MFMA2(A, Bv, ACC)                                        \
  ACC = __builtin_amdgcn_mfma_f64_16x16x4f64((A).x, (Bv).x, ACC, 0, 0, 0);  \
  ACC = __builtin_amdgcn_mfma_f64_16x16x4f64((A).y, (Bv).y, ACC, 0, 0, 0)

// 16 rows of the image x NC column blocks of the tile: `arow` = this lane's row at its lane group's k offset, `brow` = its
// sample of column block 0 likewise (column block c: + 16 c ks).  Chunks of four groups (32 k): the pieces of W of chunk
// c + 1 are in flight while the MFMAs of chunk c run; what is left of K beyond whole chunks (at most three groups) follows
// one group at a time.  Groups alternate between the two chains of every column block; out = even chain + odd chain.
template <int NC>
__device__ __forceinline__ void block_product(const double* __restrict__ arow, const double* brow, const int ks,
                                              const int groups, f64x4 (&out)[NC]) {
  f64x4 acc[NC][2];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[c][h][i] = 0.0;
  const int chunks = groups >> 2;
  if (chunks > 0) {
    f64x2 a[4], an[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) a[g] = *reinterpret_cast<const f64x2*>(arow + 8 * g);
    for (int ch = 0; ch + 1 < chunks; ++ch) {
#pragma unroll
      for (int g = 0; g < 4; ++g) an[g] = *reinterpret_cast<const f64x2*>(arow + 32 * (ch + 1) + 8 * g);
      f64x2 b[NC][4];
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) b[c][g] = *reinterpret_cast<const f64x2*>(brow + 16 * c * ks + 32 * ch + 8 * g);
      __builtin_amdgcn_sched_barrier(0);        // (the scheduler otherwise sinks the loads to their use: no prefetch left)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int c = 0; c < NC; ++c) { RAYEN_WF64_MFMA2(a[g], b[c][g], acc[c][g & 1]); }
#pragma unroll
      for (int g = 0; g < 4; ++g) a[g] = an[g];
    }
    f64x2 b[NC][4];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) b[c][g] = *reinterpret_cast<const f64x2*>(brow + 16 * c * ks + 32 * (chunks - 1) + 8 * g);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int c = 0; c < NC; ++c) { RAYEN_WF64_MFMA2(a[g], b[c][g], acc[c][g & 1]); }
  }
  for (int g = 4 * chunks; g < groups; ++g) {
    const f64x2 a = *reinterpret_cast<const f64x2*>(arow + 8 * g);
    if (g & 1) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const f64x2 b = *reinterpret_cast<const f64x2*>(brow + 16 * c * ks + 8 * g);
        RAYEN_WF64_MFMA2(a, b, acc[c][1]);
      }
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const f64x2 b = *reinterpret_cast<const f64x2*>(brow + 16 * c * ks + 8 * g);
        RAYEN_WF64_MFMA2(a, b, acc[c][0]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) out[c][i] = acc[c][0][i] + acc[c][1][i];
}

}  // namespace rayen
