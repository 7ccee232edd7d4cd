// The fused wide backward (rayen_wide_fused_bwd.hip): its LDS plan, its images' shapes and the workspace of the grouping by
// active constraint, stated once.  Plain integers, no HIP type: any C++ compiler takes this header alone
// (tests/test_wide_fused_bwd_host.py does).
//
// A workgroup of four waves owns 32 samples.  LDS, in 4-byte words:
//     region     the larger of
//                  g tile   [32][gs]   gs = ke + 4, ke = k rounded up to 8 -- only for sets with equality constraints
//                                      (u = NA_E' g has K = k); dead once u is formed
//                  v tile   [32][ks]   ks = kp + 4, kp = n rounded up to 8 (the forward's tile), followed by
//                  T tile   [32][ts]   ts = rp + 4, rp = the rows of the widest QUAD_FAC / SOC segment rounded up to 8
//                                      (0 rows: no tile).  Dense QUAD_SYM segments need none: their coefficients are v.
//                (ks / 4, gs / 4 and ts / 4 are odd: the forward's bank argument)
//     scratch    kWideFusedBwdScratch words: [4 waves][32] partial sums, and [32] each of cr, br, the active non-linear
//                segment, coef, kappa and the sample's row of the batch
//
// Images: the forward's row-major W_ext ([rows_pad][kp]) for T = W_seg v, and TRANSPOSED ones for the products whose K is a
// row index -- NA_E' as [np][ke] (np = n rounded up to 32; u = NA_E' g) and every non-linear segment d as [np][rp_d]
// (row j holds W[row0 + r][j], r < nrows; rp_d = nrows rounded up to 8) -- zero in every padded row and column, so that
// both products run the one loop of rayen_wide_fused_common.h.
//
// Grouping: key 0 = not clipped or clipped by a linear row, 1 + d = clipped by the d-th non-linear segment.  The workspace
// holds n_keys counters (which the scan turns into bucket cursors) and the permutation [B], int32 both.
#pragma once

#include <stdint.h>

namespace rayen {

constexpr int kWideFusedBwdMaxN = 1024;
constexpr int64_t kWideFusedBwdLds = 160 * 1024 - 256;
constexpr int32_t kWideFusedBwdScratch = 10 * 32;

struct WideFusedBwdPlan {
  int32_t kp, ks;            // K of the products over n, the v tile's stride
  int32_t ke, gs;            // K of u = NA_E' g and the g tile's stride (0, 0 with NA_E = I)
  int32_t rp, ts;            // the widest FAC / SOC segment's K, the T tile's stride (0, 0: none)
  int32_t np;                // rows of the transposed images
  int32_t region_words;
  int64_t lds_bytes;
  int32_t served;
};

inline int32_t wide_fused_bwd_pad8(const int32_t x) { return (x + 7) / 8 * 8; }

// `widest_t`: rows of the widest QUAD_FAC / SOC segment (0: none)
inline WideFusedBwdPlan wide_fused_bwd_plan(const int32_t n, const int32_t k, const int32_t out_identity, const int32_t widest_t) {
  WideFusedBwdPlan p;
  p.kp = wide_fused_bwd_pad8(n);
  p.ks = p.kp + 4;
  p.ke = out_identity ? 0 : wide_fused_bwd_pad8(k);
  p.gs = out_identity ? 0 : p.ke + 4;
  p.rp = widest_t > 0 ? wide_fused_bwd_pad8(widest_t) : 0;
  p.ts = widest_t > 0 ? p.rp + 4 : 0;
  p.np = (n + 31) / 32 * 32;
  const int64_t g_words = (int64_t)32 * p.gs, vt_words = (int64_t)32 * p.ks + (int64_t)32 * p.ts;
  const int64_t region = g_words > vt_words ? g_words : vt_words;
  p.lds_bytes = 4 * (region + kWideFusedBwdScratch);
  p.served = (n >= 1 && n <= kWideFusedBwdMaxN && k >= 1 && widest_t >= 0 && widest_t <= (1 << 24) && k <= (1 << 24) &&
              p.lds_bytes <= kWideFusedBwdLds) ? 1 : 0;
  p.region_words = p.served ? (int32_t)region : 0;
  return p;
}

// the grouping's workspace: cursors [n_keys] at byte 0, the permutation [B] at wide_fused_bwd_perm_offset
inline int64_t wide_fused_bwd_perm_offset(const int64_t n_keys) { return (4 * n_keys + 255) / 256 * 256; }
inline int64_t wide_fused_bwd_workspace(const int64_t n_nonlinear, const int64_t B) {
  if (n_nonlinear < 2 || B <= 0) return 0;          // one bucket beside key 0: every tile walks at most that one segment
  return wide_fused_bwd_perm_offset(n_nonlinear + 1) + 4 * B;
}

// The scan of the bucket counts, as the kernel's workgroup of `threads` does it: thread t owns the contiguous chunk
// [chunk t, chunk (t + 1)) of the keys, chunk = ceil(n_keys / threads).  Host restatement for the tests; counts -> cursors.
inline void wide_fused_bwd_scan(int32_t* counts, const int64_t n_keys, const int32_t threads) {
  const int64_t chunk = (n_keys + threads - 1) / threads;
  int64_t base = 0;
  for (int32_t t = 0; t < threads; ++t) {
    int64_t sum = 0;
    for (int64_t i = chunk * t; i < chunk * (t + 1) && i < n_keys; ++i) {
      const int32_t c = counts[i];
      counts[i] = (int32_t)(base + sum);
      sum += c;
    }
    base += sum;
  }
}

}  // namespace rayen
