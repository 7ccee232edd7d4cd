// The fused wide forward in fp64 (rayen_wide_fused64.hip): the block plan of a set, stated once.  Plain integers, no HIP
// type: any C++ compiler takes this header alone (tests/test_wide_fused64_host.py does).  The structure is that of
// rayen_wide_fused_layout.h (whose segment records and rule of dealing blocks to waves it uses) at the geometry of
// v_mfma_f64_16x16x4_f64:
//
// W_ext = [W ; NA_E] is cut into BLOCKS of 16 rows, the two parts apart: the n_rows rows of W padded to a multiple of 16
// (nb_w blocks), then -- only for sets with equality constraints -- the k rows of NA_E padded the same way (nb_e blocks).
// The image is row-major, [rows_pad][kp] doubles with kp = n rounded up to 8 (eight k per 16-byte piece over the four lane
// groups), zero in every padded row and column.  The four waves of a workgroup split each part into contiguous runs of
// blocks: wave w owns blocks [nb w / 4, nb (w + 1) / 4).
//
// A workgroup owns a tile of S samples: 32 where the LDS below fits (a wave then keeps two column blocks of 16 samples and
// every piece of W it reads feeds both), otherwise 16.  The caller may force S (16 or 32; 0 leaves the choice to the plan):
// a forced 32 that does not fit is not served.
//
// LDS of a workgroup, in 8-byte words:
//     v tile     [S][ks]    ks = kp + 2: sample s at s * ks (ks / 2 is odd: the 16-byte pieces of the sixteen samples of a
//                           column block fall into sixteen different groups of four banks)
//     scratch    per segment, at part_off: [waves of the segment][slots][S] (slots: 2 for linear rows, max and row; else 1)
//                and at aux_off: [aux rows: 1 for a quadratic, 2 for a cone, 0 for linear rows][S]
//     step       [2][S]     1 / max(1, kappa) and the NaN carry of every sample
#pragma once

#include <stdint.h>

#include "rayen_wide_fused_layout.h"

namespace rayen {

constexpr int kWideFused64Block = 16;                        // rows of a block = samples of a column block
constexpr int kWideFused64MaxN = 1024;
constexpr int64_t kWideFused64Lds = 160 * 1024 - 256;        // what a workgroup may ask for

struct WideFused64Plan {
  int32_t n, kp, ks;
  int32_t samples;                      // S: 16 or 32
  int32_t rows_w_pad, nb_w;             // W: rows padded to 16, blocks
  int32_t rows_e_pad, nb_e;             // NA_E (0 with NA_E = I)
  int32_t rows_pad;                     // rows of the image
  int32_t scratch_words;                // 8-byte words
  int64_t tile_bytes, lds_bytes;
  int32_t served;                       // n within the envelope and lds_bytes within kWideFused64Lds
};

inline int32_t wide_fused64_pad16(const int32_t rows) { return (rows + 15) / 16 * 16; }

// the segments' scratch of a tile of S samples, in 8-byte words; `seg_plans` (n_seg records, may be null) receives the plans
inline int64_t wide_fused64_scratch(const int32_t nb_w, const int32_t S, const WideFusedSegIn* segs, const int32_t n_seg,
                                    WideFusedSegPlan* seg_plans) {
  int64_t words = 0;
  for (int32_t g = 0; g < n_seg; ++g) {
    WideFusedSegPlan s;
    s.first_block = segs[g].nrows > 0 ? segs[g].row0 / kWideFused64Block : 0;
    s.last_block = segs[g].nrows > 0 ? (segs[g].row0 + segs[g].nrows - 1) / kWideFused64Block : -1;
    s.wave_first = segs[g].nrows > 0 ? wide_fused_wave_of(nb_w, s.first_block) : 0;
    s.wave_last = segs[g].nrows > 0 ? wide_fused_wave_of(nb_w, s.last_block) : -1;
    s.part_off = (int32_t)words;
    words += (int64_t)(s.wave_last - s.wave_first + 1) * segs[g].slots * S;
    s.aux_off = (int32_t)words;
    words += (int64_t)segs[g].naux * S;
    if (seg_plans != nullptr) seg_plans[g] = s;
    if (words > (int64_t)1 << 28) break;        // (far beyond LDS: not served, and no overflow)
  }
  return words;
}

// Plans a set of n variables, k outputs and n_rows rows of W for a tile of `samples` samples (0: 32 where it fits, else 16).
inline WideFused64Plan wide_fused64_plan(const int32_t n, const int32_t k, const int32_t n_rows, const int32_t out_identity,
                                         const WideFusedSegIn* segs, const int32_t n_seg, WideFusedSegPlan* seg_plans,
                                         const int32_t samples) {
  WideFused64Plan p;
  p.n = n;
  p.kp = wide_fused_kp(n);
  p.ks = p.kp + 2;
  p.rows_w_pad = wide_fused64_pad16(n_rows);
  p.nb_w = p.rows_w_pad / kWideFused64Block;
  p.rows_e_pad = out_identity ? 0 : wide_fused64_pad16(k);
  p.nb_e = p.rows_e_pad / kWideFused64Block;
  p.rows_pad = p.rows_w_pad + p.rows_e_pad;
  const bool envelope = n >= 1 && n <= kWideFused64MaxN && k >= 1 && (samples == 0 || samples == 16 || samples == 32);
  p.samples = 0;
  p.scratch_words = 0;
  p.tile_bytes = p.lds_bytes = 0;
  p.served = 0;
  for (int32_t S = (samples == 16 ? 16 : 32); S >= 16; S -= 16) {
    const int64_t words = wide_fused64_scratch(p.nb_w, S, segs, n_seg, seg_plans);
    p.samples = S;
    p.scratch_words = (int32_t)words;
    p.tile_bytes = (int64_t)8 * S * p.ks;
    p.lds_bytes = p.tile_bytes + 8 * words + 8 * 2 * S;
    p.served = (envelope && p.lds_bytes <= kWideFused64Lds) ? 1 : 0;
    if (p.served || samples == 16 || samples == 32) break;        // (a forced S is the plan's, whether it fits or not)
  }
  return p;
}

}  // namespace rayen
