// The re-laying of a projection program's rows for the fp64 tile kernel (rayen_proj_tile64.hip), its instances and its LDS
// bytes: plain integers, no HIP type (tests/tile64_layout_formulas.py restates all of it; tests/test_proj_tile64_host.py
// holds rayen_proj_tile64_layout against that).  rayen_proj_tile.hip's tile_layout() with blocks of 16 rows:
//
// nb = the smallest number of blocks per wave at which this holds: the cones, in order, go to waves 0, 1, .. (a cone that no
// longer fits the wave's 16 nb rows opens the next wave); the orthant rows then fill the blocks the cones left, wave 0
// first.  A wave's range: its cone blocks (its cones back to back, then zero pads), then its orthant blocks (pads at the
// end).  A cone never crosses two waves.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rayen {
namespace tile64 {

constexpr int kWaves = 4;
constexpr int kBlock = 16;                    // rows of a block = samples of a tile
constexpr int kMaxN = 64;
constexpr int kMaxCones = 4096;               // the cone table is device memory: this bounds its size only
constexpr int kBlockLds = kBlock * kBlock * 8;        // bytes of one block's LDS image, and of one block of registers
constexpr int kFixedLds = 1024 + 256;         // the stop maxima [4][2][16] (64 bits), the interior flags [4][16]; perm [Mp] follows
constexpr size_t kLdsLimit = 160 * 1024 - 256;        // (rayen_side_layout.h's kLdsBudget, less the static variables' share)

// blocks per wave by n: v and p take 16 registers a block, x / xt / G'u 8 a block of n.  The largest instances keep p of
// their last blocks in LDS (parked_of), or they would spill.
inline int max_blocks(int n) { return n <= 32 ? 24 : 20; }
inline int instance_nx(int n) { return n <= 32 ? 2 : 4; }                 // blocks of 16 of n the instance is built for
inline int instance_blocks(int nb, int nxi) { return nb <= 4 ? 4 : nb <= 12 ? 12 : nxi == 2 ? 24 : 20; }
constexpr int parked_of(int NB) { return NB > 20 ? 6 : NB == 20 ? 2 : 0; }
constexpr int kMaxRows = kWaves * kBlock * 24;

struct Layout {
  int Mp = 0, nb = 0;                         // padded rows; blocks of the fullest wave
  int first_block[kWaves + 1] = {};
  int cone_blocks[kWaves] = {}, cone_first[kWaves] = {}, cone_count[kWaves] = {};
  std::vector<int> perm;                      // [Mp]: original row, -1 for a pad
  std::vector<int> cone_row0, cone_rows;      // per cone: first row inside its wave's cone image, rows
};

inline bool layout(int m_lin, const int32_t* soc_rows, int n_soc, int nb_limit, Layout* out) {
  for (int nb = 1; nb <= nb_limit; ++nb) {
    const int cap = kBlock * nb;
    int used[kWaves] = {}, count[kWaves] = {}, w = 0;
    bool ok = true;
    for (int c = 0; c < n_soc && ok; ++c) {
      while (w < kWaves && used[w] + soc_rows[c] > cap) ++w;
      if (w == kWaves) { ok = false; break; }
      used[w] += soc_rows[c];
      ++count[w];
    }
    if (!ok) continue;
    int64_t room = 0;
    for (int k = 0; k < kWaves; ++k) room += cap - kBlock * ((used[k] + kBlock - 1) / kBlock);
    if (room < m_lin) continue;
    Layout& L = *out;
    L = Layout();
    L.nb = nb;
    int cone = 0, orth = 0, at = 0;
    for (int k = 0; k < kWaves; ++k) {
      L.first_block[k] = at / kBlock;
      L.cone_blocks[k] = (used[k] + kBlock - 1) / kBlock;
      L.cone_first[k] = cone;
      L.cone_count[k] = count[k];
      int local = 0;
      for (int c = 0; c < count[k]; ++c, ++cone) {
        L.cone_row0.push_back(local);
        L.cone_rows.push_back(soc_rows[cone]);
        for (int r = 0; r < soc_rows[cone]; ++r) L.perm.push_back(-2);      // (numbered below: the cones follow the orthant rows)
        local += soc_rows[cone];
      }
      for (; local < kBlock * L.cone_blocks[k]; ++local) L.perm.push_back(-1);
      const int take = std::min(m_lin - orth, cap - kBlock * L.cone_blocks[k]);
      for (int r = 0; r < take; ++r) L.perm.push_back(orth++);
      for (int r = take; r % kBlock != 0; ++r) L.perm.push_back(-1);
      at = (int)L.perm.size();
    }
    L.first_block[kWaves] = at / kBlock;
    L.Mp = at;
    int row = m_lin;
    for (int& p : L.perm)
      if (p == -2) p = row++;
    return true;
  }
  return false;
}

// dynamic LDS of a launch: the cone blocks' images (shared with the four waves' G'u partial sums), v*'s cone images
// (backward), 2q + w0, the fixed part, perm, the parked blocks of p
inline size_t lds_bytes(const Layout& L, int n, bool backward) {
  const int nxi = instance_nx(n);
  const size_t parked = (size_t)kWaves * parked_of(instance_blocks(L.nb, nxi)) * kBlockLds;
  int cone_blocks = 0;
  for (int k = 0; k < kWaves; ++k) cone_blocks += L.cone_blocks[k];
  const size_t shared = std::max((size_t)cone_blocks * kBlockLds, (size_t)kWaves * nxi * kBlockLds);
  return shared + (backward ? (size_t)cone_blocks * kBlockLds : 0) + (size_t)nxi * kBlockLds + kFixedLds + (size_t)L.Mp * 4 + parked;
}

// tile64_served(): the one rule, by sizes alone.  1 <= n <= 64; no PSD block (the cones' rows and the orthant rows are all
// of m); the rows, re-laid, in max_blocks(n) blocks a wave (the register file); the backward's LDS within the limit.
inline bool served(int n, int m, int m_lin, const int32_t* soc_rows, int n_soc, Layout* L) {
  if (n < 1 || n > kMaxN || m < 1 || n_soc < 0 || n_soc > kMaxCones || m_lin < 0) return false;
  int64_t rows = m_lin;
  for (int c = 0; c < n_soc; ++c) {
    if (soc_rows[c] < 1) return false;
    rows += soc_rows[c];
  }
  if (rows != m || rows > kMaxRows) return false;                 // (rows left over: a PSD block)
  if (!layout(m_lin, soc_rows, n_soc, max_blocks(n), L)) return false;
  return lds_bytes(*L, n, true) <= kLdsLimit;
}

}  // namespace tile64
}  // namespace rayen
