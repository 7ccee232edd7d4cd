// The fp64 tile soft cost (rayen_cost_tile64.hip): the image of a set's stacked rows in BLOCKS of 16 rows, the place of an
// element inside a block, and how the blocks are cut into windows, stated once.  Plain integers, no HIP type: any C++
// compiler takes this header alone (tests/test_cost_tile64_host.py does).
//
// Items, in the stacked order: the run of linear rows (ceil(m1 / 16) blocks, may be cut between any two blocks), each
// quadratic (the ceil(k / 16) blocks of its symmetrised P, one form q; never cut), each cone (ceil(rows / 16) blocks of M,
// one form c; never cut), the run of equality rows (as the linear one).  A WINDOW is a self-contained image (8-byte words)
//     W [nb][16 * K] | rowc [nb][16] | colv [nf][KF] | fconst [nb] | desc [nb][8 ints]        KF = max(K, 16)
// of at most `window_bytes` bytes; K is k padded to 8, 16, 32 or 64.  The partition is greedy, as in
// rayen_cost_stream_layout.h: an item that does not fit what is left of the window closes it, a run fills the window to the
// last block that fits.
//
// Inside a block the element (row m, column c) sits at word cost_tile64_slot(m, c): one image serves both products of the
// kernel without a bank conflict.  A ds_read_b64 is served per half wave (32 lanes), 32 words of 8 bytes wide, so the five
// low bits of the slot must take 32 different values over the lanes of a half:
//     first product  (step j, lane = m + 16 g reads (m, 4 j + g)):   a half varies m (4 bits) and bit 0 of c
//     second product (step i, lane = c' + 16 g reads (4 i + g, c')): a half varies c' (4 bits) and bit 0 of m
// low bits = m0 | c0 << 1 | ((m >> 1) ^ (c >> 1) & 7) << 2 are a bijection of either; the high bits are c >> 1.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rayen {

constexpr int kCostTile64Rows = 16;                           // rows of a block, samples of a column block
constexpr int kCostTile64MaxK = 64;
constexpr int64_t kCostTile64Lds = 160 * 1024;                // kLdsBudget (rayen_side_layout.h)
constexpr int64_t kCostTile64Window = kCostTile64Lds / 2 / 16 * 16;      // the default window: two buffers in LDS
constexpr int64_t kCostTile64MaxImage = (int64_t)1 << 30;     // table and all windows together
constexpr int kCostTile64TableWords = 8;                      // ints per window in the table in front of the windows

// k padded to the width of a kernel instance; 0 outside 1 .. 64
inline int cost_tile64_width(const int k) {
  if (k < 1 || k > kCostTile64MaxK) return 0;
  return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64;
}
inline int cost_tile64_form_width(const int K) { return K < 16 ? 16 : K; }
inline int cost_tile64_blocks(const int64_t rows) { return (int)((rows + kCostTile64Rows - 1) / kCostTile64Rows); }

// word of (row m of the block, column c) inside the block's 16 * K words (constexpr: host and device code share it)
constexpr int cost_tile64_slot(const int m, const int c) {
  return (m & 1) | ((c & 1) << 1) | ((((m >> 1) ^ (c >> 1)) & 7) << 2) | ((c >> 1) << 5);
}

struct CostTile64Item {
  int32_t blocks, forms, splittable;
};
struct CostTile64Piece {
  int32_t item, block0, blocks;
};
struct CostTile64Window {
  int32_t piece0, pieces, blocks, forms;
  int64_t bytes;
};

// bytes of a window of nb blocks and nf forms
inline int64_t cost_tile64_bytes(const int64_t nb, const int64_t nf, const int K) {
  return (8 * (nb * (16 * K + 16 + 1 + 4) + nf * cost_tile64_form_width(K)) + 15) / 16 * 16;
}

// 0 = the default; anything else must be a positive multiple of 16 up to the default
inline bool cost_tile64_window_ok(const int64_t window_bytes) {
  return window_bytes == 0 || (window_bytes > 0 && window_bytes % 16 == 0 && window_bytes <= kCostTile64Window);
}

// Cuts `n_items` items into windows of at most `window_bytes` bytes.  Writes up to `cap_w` windows and `cap_p` pieces
// (either array may be null with a capacity of 0: a counting call) and returns the number of windows, with the number of
// pieces and the bytes of all windows in *n_pieces / *total_bytes (each may be null).  -1: an item does not fit a window.
inline int64_t cost_tile64_partition(const CostTile64Item* items, const int64_t n_items, const int K, const int64_t window_bytes,
                                     CostTile64Window* windows, const int64_t cap_w, CostTile64Piece* pieces,
                                     const int64_t cap_p, int64_t* n_pieces, int64_t* total_bytes) {
  int64_t nw = 0, np = 0, total = 0;
  CostTile64Window cur = {0, 0, 0, 0, 0};
  auto close = [&]() {
    cur.bytes = cost_tile64_bytes(cur.blocks, cur.forms, K);
    if (windows != nullptr && nw < cap_w) windows[nw] = cur;
    total += cur.bytes;
    ++nw;
    cur = CostTile64Window{(int32_t)np, 0, 0, 0, 0};
  };
  auto add = [&](const int64_t item, const int32_t block0, const int32_t blocks, const int32_t forms) {
    if (pieces != nullptr && np < cap_p) pieces[np] = CostTile64Piece{(int32_t)item, block0, blocks};
    ++np;
    cur.pieces += 1;
    cur.blocks += blocks;
    cur.forms += forms;
  };
  auto fits = [&](const int64_t blocks, const int64_t forms) {
    return cost_tile64_bytes(cur.blocks + blocks, cur.forms + forms, K) <= window_bytes;
  };
  for (int64_t it = 0; it < n_items; ++it) {
    const CostTile64Item& m = items[it];
    if (m.blocks <= 0) continue;
    if (!m.splittable) {
      if (!fits(m.blocks, m.forms)) {
        if (cur.pieces > 0) close();
        if (!fits(m.blocks, m.forms)) return -1;
      }
      add(it, 0, m.blocks, m.forms);
      continue;
    }
    int32_t done = 0;
    while (done < m.blocks) {
      int32_t n = 0;      // the most blocks of the run that fit what is left of the window
      while (n < m.blocks - done && fits(n + 1, 0)) ++n;
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

// The envelope, by sizes alone: 1 <= k <= 64, at least one item, every item within one window, the table and all windows
// within 1 GiB.  A cone of any number of rows that fits a window is served (beyond one block its products are computed
// again for the gradient, rayen_cost_tile64.hip).  window_bytes as cost_tile64_window_ok takes it.
inline bool cost_tile64_served(const int k, const CostTile64Item* items, const int64_t n_items, const int64_t window_bytes) {
  const int K = cost_tile64_width(k);
  if (K == 0 || !cost_tile64_window_ok(window_bytes)) return false;
  int64_t total = 0;
  const int64_t nw = cost_tile64_partition(items, n_items, K, window_bytes == 0 ? kCostTile64Window : window_bytes, nullptr, 0,
                                           nullptr, 0, nullptr, &total);
  return nw > 0 && nw * kCostTile64TableWords * 4 + total <= kCostTile64MaxImage;
}

}  // namespace rayen
