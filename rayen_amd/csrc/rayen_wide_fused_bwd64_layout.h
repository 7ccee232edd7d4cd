// The fused wide backward in fp64 (rayen_wide_fused_bwd64.hip): its LDS plan and its images' shapes, stated once.  Plain
// integers, no HIP type: any C++ compiler takes this header alone (tests/test_wide_fused_bwd64_host.py does).  It is the plan
// of rayen_wide_fused_bwd_layout.h (whose padding rule and grouping workspace -- int32 cursors and permutation,
// wide_fused_bwd_workspace, wide_fused_bwd_perm_offset -- it uses as they are) at the geometry of v_mfma_f64_16x16x4_f64.
//
// A workgroup of four waves owns S samples: 32 where the LDS below fits (a wave then keeps two column blocks of 16 samples
// and every piece of an image it reads feeds both), otherwise 16.  The caller may force S (16 or 32; 0 leaves the choice to
// the plan): a forced 32 that does not fit is not served -- the rule of rayen_wide_fused64_layout.h.  LDS, in 8-byte words:
//     region     the larger of
//                  g tile   [S][gs]    gs = ke + 2, ke = k rounded up to 8 -- only for sets with equality constraints
//                                      (u = NA_E' g has K = k); dead once u is formed
//                  v tile   [S][ks]    ks = kp + 2, kp = n rounded up to 8 (the forward's tile), followed by
//                  T tile   [S][ts]    ts = rp + 2, rp = the rows of the widest QUAD_FAC / SOC segment rounded up to 8
//                                      (0 rows: no tile).  Dense QUAD_SYM segments need none: their coefficients are v.
//                (ks / 2, gs / 2 and ts / 2 are odd: the fp64 forward's bank argument -- the 16-byte pieces of the sixteen
//                samples of a column block fall into sixteen different groups of four banks)
//     scratch    10 S words: [4 waves][S] partial sums, and [S] each of cr, br, the active non-linear segment, coef, kappa
//                and one spare
//
// Images: the fp64 forward's row-major W_ext ([rows_pad][kp], rows padded to 16) for T = W_seg v, and TRANSPOSED ones for
// the products whose K is a row index -- NA_E' as [np][ke] (np = n rounded up to 16; u = NA_E' g) and every non-linear
// segment d as [np][rp_d] (row j holds W[row0 + r][j], r < nrows; rp_d = nrows rounded up to 8) -- zero in every padded row
// and column, so that both products run the one loop of rayen_wide_fused64_common.h.
#pragma once

#include <stdint.h>

#include "rayen_wide_fused_bwd_layout.h"

namespace rayen {

constexpr int kWideFusedBwd64MaxN = 1024;
constexpr int64_t kWideFusedBwd64Lds = 160 * 1024 - 256;

struct WideFusedBwd64Plan {
  int32_t kp, ks;            // K of the products over n, the v tile's stride
  int32_t ke, gs;            // K of u = NA_E' g and the g tile's stride (0, 0 with NA_E = I)
  int32_t rp, ts;            // the widest FAC / SOC segment's K, the T tile's stride (0, 0: none)
  int32_t np;                // rows of the transposed images
  int32_t samples;           // S: 16 or 32
  int32_t region_words;      // 8-byte words (0: not served)
  int64_t lds_bytes;
  int32_t served;            // n within the envelope and lds_bytes within kWideFusedBwd64Lds
};

inline int32_t wide_fused_bwd64_scratch(const int32_t S) { return 10 * S; }

// `widest_t`: rows of the widest QUAD_FAC / SOC segment (0: none); `samples`: 0 (32 where it fits, else 16), or 16 / 32 forced
inline WideFusedBwd64Plan wide_fused_bwd64_plan(const int32_t n, const int32_t k, const int32_t out_identity,
                                                const int32_t widest_t, const int32_t samples) {
  WideFusedBwd64Plan p;
  p.kp = wide_fused_bwd_pad8(n);
  p.ks = p.kp + 2;
  p.ke = out_identity ? 0 : wide_fused_bwd_pad8(k);
  p.gs = out_identity ? 0 : p.ke + 2;
  p.rp = widest_t > 0 ? wide_fused_bwd_pad8(widest_t) : 0;
  p.ts = widest_t > 0 ? p.rp + 2 : 0;
  p.np = (n + 15) / 16 * 16;
  const bool envelope = n >= 1 && n <= kWideFusedBwd64MaxN && k >= 1 && widest_t >= 0 && widest_t <= (1 << 24) &&
                        k <= (1 << 24) && (samples == 0 || samples == 16 || samples == 32);
  p.samples = 0;
  p.region_words = 0;
  p.lds_bytes = 0;
  p.served = 0;
  for (int32_t S = (samples == 16 ? 16 : 32); S >= 16; S -= 16) {
    const int64_t g_words = (int64_t)S * p.gs, vt_words = (int64_t)S * p.ks + (int64_t)S * p.ts;
    const int64_t region = g_words > vt_words ? g_words : vt_words;
    p.samples = S;
    p.lds_bytes = 8 * (region + wide_fused_bwd64_scratch(S));
    p.served = (envelope && p.lds_bytes <= kWideFusedBwd64Lds) ? 1 : 0;
    p.region_words = p.served ? (int32_t)region : 0;
    if (p.served || samples == 16 || samples == 32) break;        // (a forced S is the plan's, whether it fits or not)
  }
  return p;
}

}  // namespace rayen
