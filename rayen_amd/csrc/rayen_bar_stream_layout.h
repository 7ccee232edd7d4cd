// The streamed Bar kernels (rayen_bar_stream.hip): how the image of G = NA_E [V R] is walked in windows, stated once.
// Plain integers, no HIP type: any C++ compiler takes this header alone (tests/test_bar_stream_host.py does).
//
// The image is the pack's own ([round_up(m, 4) + 1][K] elements, generator j in row gen_slot(j), yp in the last row).
// gen_slot permutes only within an aligned GROUP of four generators, and a group is what a row's 16-byte PIECE of q
// multiplies: piece p of a row holds the logits of generators 4p .. 4p + 3, whose coefficients are the image's rows
// 4p .. 4p + 3 in some order.  A WINDOW is `g` consecutive groups: a contiguous slice of g * 4 * K * elem bytes of the image,
// the last one possibly shorter.  Piece p is in window p / g.  yp's row is in no window: it has an LDS slot of its own.
//
// A workgroup's LDS: the slot of yp (kBarStreamYpBytes) | buffer 0 | buffer 1 (one buffer when the set is one window).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rayen {

constexpr int64_t kBarStreamLds = 160 * 1024;              // kLdsBudget (rayen_side_layout.h)
constexpr int64_t kBarStreamYpBytes = 64 * 8;              // yp's slot: K <= 64 elements of at most 8 bytes
constexpr int kBarStreamThreads = 512;                     // a workgroup (rayen_bar.hip: kThreads)
// the largest window two buffers and yp's slot leave room for, in whole 16-byte pieces
constexpr int64_t kBarStreamMaxWindow = (kBarStreamLds - kBarStreamYpBytes) / 2 / 16 * 16;
// the default window: the fastest of 20, 40 and 80 KiB on the 12-D box in fp32 (profiles/bench/bar_stream.txt); three
// workgroups' buffers fit a CU's LDS
constexpr int64_t kBarStreamWindow = 20 * 1024;
static_assert(kBarStreamWindow % 16 == 0 && kBarStreamWindow <= kBarStreamMaxWindow, "two buffers and yp's slot fit LDS");

// 0 = the default; anything else must be a positive multiple of 16 up to the default
inline bool bar_stream_window_ok(const int64_t window_bytes) {
  return window_bytes == 0 || (window_bytes > 0 && window_bytes % 16 == 0 && window_bytes <= kBarStreamWindow);
}

// groups of four generators per window (rounded down to whole groups); 0: the window does not hold one group, an error
inline int64_t bar_stream_groups(const int64_t window_bytes, const int K, const int64_t elem) {
  const int64_t w = window_bytes == 0 ? kBarStreamWindow : window_bytes;
  return w / (4 * (int64_t)K * elem);
}

constexpr int64_t bar_stream_pieces(const int64_t m) { return (m + 3) / 4; }

// windows of a set of m generators at g groups per window; the window of piece p
constexpr int64_t bar_stream_windows(const int64_t m, const int64_t g) { return (bar_stream_pieces(m) + g - 1) / g; }
constexpr int64_t bar_stream_window_of(const int64_t piece, const int64_t g) { return piece / g; }

// bytes of a buffer (the largest window of the set) and of a workgroup's LDS
inline int64_t bar_stream_buffer_bytes(const int64_t m, const int64_t g, const int K, const int64_t elem) {
  const int64_t pieces = bar_stream_pieces(m);
  return (pieces < g ? pieces : g) * 4 * K * elem;
}
inline int64_t bar_stream_lds_bytes(const int64_t m, const int64_t g, const int K, const int64_t elem) {
  return kBarStreamYpBytes + (bar_stream_windows(m, g) > 1 ? 2 : 1) * bar_stream_buffer_bytes(m, g, K, elem);
}

// The window sequences of one pass over a workgroup's rows.  Both are two runs of consecutive windows:
//   forward:  the windows of the vertex pieces [0, pv), then the windows of the ray pieces [pr, pieces)
//   backward: the windows of the vertex pieces (sum and <lambda, g>), then every window from 0 (grad_q)
// pv = ceil(nv / 4), pr = nv / 4: with nv % 4 != 0 and rays, piece pr is in both runs.  A step whose window is the previous
// step's finds it in LDS and copies nothing (so does the first step of the next pass where the sequence is one window).
// (constexpr: the kernels call these too.)
struct BarStreamSeq {
  int32_t first_end;       // the first run: windows [0, first_end)
  int32_t second_begin;    // the second run: windows [second_begin, windows)
  int32_t windows;
};
constexpr int32_t bar_stream_seq_steps(const BarStreamSeq& s) { return s.first_end + (s.windows - s.second_begin); }
constexpr int32_t bar_stream_seq_window(const BarStreamSeq& s, const int32_t step) {
  return step < s.first_end ? step : s.second_begin + (step - s.first_end);
}
constexpr int32_t bar_stream_vertex_windows(const int64_t nv, const int64_t g) {
  return nv > 0 ? (int32_t)(((nv + 3) / 4 - 1) / g + 1) : 0;
}
constexpr BarStreamSeq bar_stream_forward_seq(const int64_t nv, const int64_t m, const int64_t g) {
  return BarStreamSeq{bar_stream_vertex_windows(nv, g),
                      m > nv ? (int32_t)((nv / 4) / g) : (int32_t)bar_stream_windows(m, g), (int32_t)bar_stream_windows(m, g)};
}
constexpr BarStreamSeq bar_stream_backward_seq(const int64_t nv, const int64_t m, const int64_t g) {
  return BarStreamSeq{bar_stream_vertex_windows(nv, g), 0, (int32_t)bar_stream_windows(m, g)};
}

// lanes that share a row: 2^lg, about a quarter of m, at most 16 (rayen_bar.hip: group_log2)
inline int bar_stream_group_log2(const int64_t m) {
  const int64_t pieces = bar_stream_pieces(m);
  int lg = 0;
  while (((int64_t)1 << lg) < pieces && lg < 4) ++lg;
  return lg;
}

// R: the rows a lane group carries at once (R sets of accumulators in registers, R rows of q in flight), per K and
// precision: the largest of {1, 2, 4} whose kernels use no scratch and are not slower than R = 1.  Measured
// (profiles/bench/bar_stream.txt), R > 1 is slower or no faster at every K in both precisions: the registers it takes
// cost more occupancy than the image's re-reads from L2 cost time.
constexpr int bar_stream_rows(const int K, const int f64) {
  return (void)K, (void)f64, 1;
}

// rows a workgroup takes per pass over the image
inline int64_t bar_stream_rows_per_pass(const int64_t m, const int K, const int f64) {
  return (int64_t)(kBarStreamThreads >> bar_stream_group_log2(m)) * bar_stream_rows(K, f64);
}

// workgroups per CU a launch counts on: what LDS leaves room for, at most 4 (2 048 threads).  An upper bound: an instance
// that needs more than 128 registers (fp64 at K >= 32, fp32 at K = 64) is resident once or twice a CU whatever LDS allows,
// and the workgroups beyond wait their turn; the row loop is grid-stride and nothing synchronises across workgroups.
inline int64_t bar_stream_wg_per_cu(const int64_t lds_bytes) {
  const int64_t n = kBarStreamLds / lds_bytes;
  return n > 4 ? 4 : n < 1 ? 1 : n;
}

}  // namespace rayen
