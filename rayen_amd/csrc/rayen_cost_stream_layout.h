// The streamed soft cost (rayen_cost_stream.hip): how the image of a set's stacked rows is cut into windows, stated once.
// Plain integers, no HIP type: any C++ compiler takes this header alone (tests/test_cost_stream_host.py does).
//
// The image is a sequence of ITEMS in the stacked order; an item has `units` (fp32: tiles of 32 rows; fp64: rows), at most
// one `form` (the column vector of a quadratic or a cone) and is either splittable (a run of linear or of equality rows:
// it may be cut between any two units) or not (a quadratic, a cone: all of it sits in one window).  A WINDOW is a
// self-contained image in the resident layout,
//     fp32: W [nt][32][64] swizzled | rowc [nt][32] | colv [nf][64] | desc [nt][8]                  (4-byte words)
//     fp64: W [R][K] | rowc [R] | colv [nf][K] | fconst [ni] | desc [ni][8 ints]                    (8-byte words)
// of at most `window_bytes` bytes, made of PIECES: (item, first unit of the item, units).  The partition is greedy: an item
// that does not fit what is left of the window closes it; a splittable item fills the window to the last unit that fits.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rayen {

constexpr int64_t kCostStreamLds = 160 * 1024;            // kLdsBudget (rayen_side_layout.h)
constexpr int64_t kCostStreamScratch = 0;                 // LDS the streamed kernels use next to their two buffers
// the default window: half of what two buffers and the scratch leave of LDS, in whole 16-byte pieces
constexpr int64_t kCostStreamWindow = (kCostStreamLds - kCostStreamScratch) / 2 / 16 * 16;
constexpr int64_t kCostStreamMaxImage = (int64_t)1 << 30;      // all windows together

struct CostStreamItem {
  int32_t units, forms, splittable;
};
struct CostStreamPiece {
  int32_t item, unit0, units;
};
struct CostStreamWindow {
  int32_t piece0, pieces, units, forms;
  int64_t bytes;
};

// bytes of a window: fp32 of nt tiles and nf forms | fp64 of R rows of K columns, nf forms and ni items (pieces)
inline int64_t cost_stream_bytes32(const int64_t nt, const int64_t nf) { return 4 * (nt * (2048 + 32 + 8) + nf * 64); }
inline int64_t cost_stream_bytes64(const int64_t R, const int64_t nf, const int64_t ni, const int K) {
  return (8 * (R * K + R + nf * K + ni + ni * 4) + 15) / 16 * 16;
}
inline int64_t cost_stream_bytes(const int f64, const int K, const int64_t units, const int64_t forms, const int64_t pieces) {
  return f64 ? cost_stream_bytes64(units, forms, pieces, K) : cost_stream_bytes32(units, forms);
}

// the smallest window that holds any fp32 item: two tiles and a form
constexpr int64_t kCostStreamMinWindow32 = 4 * (2 * (2048 + 32 + 8) + 64);

// 0 = the default; anything else must be a positive multiple of 16 up to the default
inline bool cost_stream_window_ok(const int64_t window_bytes) {
  return window_bytes == 0 || (window_bytes > 0 && window_bytes % 16 == 0 && window_bytes <= kCostStreamWindow);
}

// Cuts `n_items` items into windows of at most `window_bytes` bytes.  Writes up to `cap_w` windows and `cap_p` pieces
// (either array may be null with a capacity of 0: a counting call) and returns the number of windows, with the number of
// pieces and the bytes of all windows in *n_pieces / *total_bytes (each may be null).  -1: an item does not fit a window.
inline int64_t cost_stream_partition(const CostStreamItem* items, const int64_t n_items, const int f64, const int K,
                                     const int64_t window_bytes, CostStreamWindow* windows, const int64_t cap_w,
                                     CostStreamPiece* pieces, const int64_t cap_p, int64_t* n_pieces, int64_t* total_bytes) {
  int64_t nw = 0, np = 0, total = 0;
  CostStreamWindow cur = {0, 0, 0, 0, 0};
  auto close = [&]() {
    cur.bytes = cost_stream_bytes(f64, K, cur.units, cur.forms, cur.pieces);
    if (windows != nullptr && nw < cap_w) windows[nw] = cur;
    total += cur.bytes;
    ++nw;
    cur = CostStreamWindow{(int32_t)np, 0, 0, 0, 0};
  };
  auto add = [&](const int64_t item, const int32_t unit0, const int32_t units, const int32_t forms) {
    if (pieces != nullptr && np < cap_p) pieces[np] = CostStreamPiece{(int32_t)item, unit0, units};
    ++np;
    cur.pieces += 1;
    cur.units += units;
    cur.forms += forms;
  };
  auto fits = [&](const int64_t units, const int64_t forms) {
    return cost_stream_bytes(f64, K, cur.units + units, cur.forms + forms, cur.pieces + 1) <= window_bytes;
  };
  for (int64_t it = 0; it < n_items; ++it) {
    const CostStreamItem& m = items[it];
    if (m.units <= 0) continue;
    if (!m.splittable) {
      if (!fits(m.units, m.forms)) {
        if (cur.pieces > 0) close();
        if (!fits(m.units, m.forms)) return -1;
      }
      add(it, 0, m.units, m.forms);
      continue;
    }
    int32_t done = 0;
    while (done < m.units) {
      int32_t n = 0;      // the most units of the run that fit what is left of the window
      while (n < m.units - done && fits(n + 1, 0)) ++n;
      if (n == 0) {
        if (cur.pieces == 0) return -1;
        close();
        continue;
      }
      add(it, done, n, 0);
      done += n;
    }
  }
  if (cur.pieces > 0) close();
  if (n_pieces != nullptr) *n_pieces = np;
  if (total_bytes != nullptr) *total_bytes = total;
  return nw;
}

}  // namespace rayen
