// The fused wide forward (rayen_wide_fused.hip): the block plan of a set, stated once.  Plain integers, no HIP type: any
// C++ compiler takes this header alone (tests/test_wide_fused_host.py does).
//
// W_ext = [W ; NA_E] is cut into BLOCKS of 32 rows, the two parts apart: the n_rows rows of W padded to a multiple of 32
// (nb_w blocks), then -- only for sets with equality constraints -- the k rows of NA_E padded the same way (nb_e blocks).
// The image is row-major, [rows_pad][kp] floats with kp = n rounded up to 8 (eight k per 16-byte load of the two half-waves),
// zero in every padded row and column.  The four waves of a workgroup split each part into CONTIGUOUS runs of blocks:
// wave w owns blocks [nb w / 4, nb (w + 1) / 4) of a part of nb blocks (computeKappa skips the second part and stays
// balanced).  A segment's rows are consecutive, so the waves that own some of them are consecutive too; each of them keeps
// ONE partial per sample for the segment (a sum; for linear rows a maximum and its row), folded over its own blocks in
// rising order, and the final pass folds the waves' partials in rising order: first to last block of the segment.
//
// LDS of a workgroup, in 4-byte words:
//     v tile     [32][ks]   ks = kp + 4: sample s at s * ks (ks / 4 is odd: eight consecutive samples' 16-byte pieces of one
//                           column group fall into eight different groups of four banks)
//     scratch    per segment, at part_off: [waves of the segment][slots][32] (slots: 2 for linear rows, max and row; else 1)
//                and at aux_off: [aux rows: 1 for a quadratic, 2 for a cone, 0 for linear rows][32]
//     step       [2][32]    1 / max(1, kappa) and the NaN carry of every sample
#pragma once

#include <stdint.h>

namespace rayen {

constexpr int kWideFusedTile = 32;                          // samples of a workgroup = rows of a block
constexpr int kWideFusedWaves = 4;
constexpr int kWideFusedMaxN = 1024;
constexpr int64_t kWideFusedLds = 160 * 1024 - 256;         // what a workgroup may ask for

struct WideFusedSegIn {      // a segment without an LMI: its rows of W, slots of a wave's partial, rows captured as they are
  int32_t row0, nrows, slots, naux;
};
struct WideFusedSegPlan {
  int32_t first_block, last_block;      // blocks of W holding the segment's rows (last < first: no row)
  int32_t wave_first, wave_last;        // owners of those two blocks
  int32_t part_off, aux_off;            // words from the start of the scratch
};
struct WideFusedPlan {
  int32_t n, kp, ks;
  int32_t rows_w_pad, nb_w;             // W: rows padded to 32, blocks
  int32_t rows_e_pad, nb_e;             // NA_E (0 with NA_E = I)
  int32_t rows_pad;                     // rows of the image
  int32_t scratch_words;
  int64_t tile_bytes, lds_bytes;
  int32_t served;                       // n within the envelope and lds_bytes within kWideFusedLds
};

inline int32_t wide_fused_pad32(const int32_t rows) { return (rows + 31) / 32 * 32; }
inline int32_t wide_fused_kp(const int32_t n) { return (n + 7) / 8 * 8; }
// first block of wave w in a part of nb blocks (w = kWideFusedWaves: nb)
inline int32_t wide_fused_block_start(const int32_t nb, const int32_t w) { return (int32_t)((int64_t)nb * w / kWideFusedWaves); }
// the wave that owns block b of a part of nb blocks
inline int32_t wide_fused_wave_of(const int32_t nb, const int32_t b) {
  for (int32_t w = 0; w < kWideFusedWaves; ++w)
    if (b >= wide_fused_block_start(nb, w) && b < wide_fused_block_start(nb, w + 1)) return w;
  return -1;
}

// Plans a set of n variables, k outputs and n_rows rows of W; `seg_plans` (n_seg records, may be null) receives the segments'.
inline WideFusedPlan wide_fused_plan(const int32_t n, const int32_t k, const int32_t n_rows, const int32_t out_identity,
                                     const WideFusedSegIn* segs, const int32_t n_seg, WideFusedSegPlan* seg_plans) {
  WideFusedPlan p;
  p.n = n;
  p.kp = wide_fused_kp(n);
  p.ks = p.kp + 4;
  p.rows_w_pad = wide_fused_pad32(n_rows);
  p.nb_w = p.rows_w_pad / 32;
  p.rows_e_pad = out_identity ? 0 : wide_fused_pad32(k);
  p.nb_e = p.rows_e_pad / 32;
  p.rows_pad = p.rows_w_pad + p.rows_e_pad;
  int64_t words = 0;
  for (int32_t g = 0; g < n_seg; ++g) {
    WideFusedSegPlan s;
    s.first_block = segs[g].nrows > 0 ? segs[g].row0 / 32 : 0;
    s.last_block = segs[g].nrows > 0 ? (segs[g].row0 + segs[g].nrows - 1) / 32 : -1;
    s.wave_first = segs[g].nrows > 0 ? wide_fused_wave_of(p.nb_w, s.first_block) : 0;
    s.wave_last = segs[g].nrows > 0 ? wide_fused_wave_of(p.nb_w, s.last_block) : -1;
    s.part_off = (int32_t)words;
    words += (int64_t)(s.wave_last - s.wave_first + 1) * segs[g].slots * 32;
    s.aux_off = (int32_t)words;
    words += (int64_t)segs[g].naux * 32;
    if (seg_plans != nullptr) seg_plans[g] = s;
    if (words > (int64_t)1 << 28) break;        // (far beyond LDS: not served, and no overflow)
  }
  p.scratch_words = (int32_t)words;
  p.tile_bytes = (int64_t)4 * 32 * p.ks;
  p.lds_bytes = p.tile_bytes + 4 * words + 4 * 2 * 32;
  p.served = (n >= 1 && n <= kWideFusedMaxN && k >= 1 && p.lds_bytes <= kWideFusedLds) ? 1 : 0;
  return p;
}

}  // namespace rayen
