// The operand images of the DC3 tile kernels (rayen_dc3_tile.hip) and the rule of what they serve: plain host code on host
// vectors, no HIP call and no HIP type (any C++ compiler takes this header alone).
//
// A product of the kernels is  OUT [32 rows x 32 samples] += M_block [32 x K] X [K x 32 samples]  by v_mfma_f32_32x32x2_f32,
// with X in accumulator layout: lane l, register i of a 32-row block of X is sample l & 31, row 8 (i >> 2) + 4 (l >> 5) +
// (i & 3).  The B operand of that MFMA is B[k = l >> 5][sample = l & 31]: register i of X IS the B operand of one k-step
// (its two half-waves hold rows r and r + 4), and the A operand of that step is M[row l & 31][column r + 4 (l >> 5)].  So
// an image stores, per lane, the four A operands of registers 4 g .. 4 g + 3 as one float4:
//   rows    [block][g < kg][lane]      -> M[32 block + (lane & 31)][8 g + 4 (lane >> 5) + e]           (M X, X of n rows)
//   columns [block][ob < nx][g < 4][lane] -> M[32 block + 8 g + 4 (lane >> 5) + e][32 ob + (lane & 31)] (M' X, X of 32 rows)
// e = 0..3, kg = ceil(n / 8), nx = ceil(n / 32); everything outside M is zero.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace rayen {

constexpr int kDc3TileMaxN = 64;
constexpr int64_t kDc3TileMaxImageBytes = (int64_t)1 << 30;      // the image is one device allocation

struct Dc3TileDims {
  int n = 0, m = 0, nq = 0, no = 0;
  int nx = 0, kg = 0, Mb = 0, Cb = 0;      // blocks of n; groups of 8 columns of n; row blocks of A1e; row blocks of C
  // offsets in floats, each a multiple of 4
  int64_t off_A = 0, off_AT = 0, off_b = 0, off_P = 0, off_PT = 0, off_q = 0, off_r = 0, off_C = 0, off_CT = 0, off_c0 = 0,
          total = 0;
};

inline Dc3TileDims dc3_tile_dims(const int n, const int m, const int nq, const int no) {
  Dc3TileDims d;
  d.n = n; d.m = m; d.nq = nq; d.no = no;
  d.nx = (n + 31) / 32; d.kg = (n + 7) / 8;
  d.Mb = (int)(((int64_t)m + 31) / 32); d.Cb = (int)(((int64_t)no + 31) / 32);
  int64_t at = 0;
  d.off_A = at;  at += (int64_t)d.Mb * d.kg * 256;            // A1e, rows
  d.off_AT = at; at += (int64_t)d.Mb * d.nx * 1024;           // A1e, columns
  d.off_b = at;  at += (int64_t)d.Mb * 32;                    // b1e [32 Mb]
  d.off_P = at;  at += (int64_t)nq * d.nx * d.kg * 256;       // Pe_i, rows (of its nx blocks)
  d.off_PT = at; at += (int64_t)nq * d.nx * d.kg * 256;       // Pe_i', rows
  d.off_q = at;  at += (int64_t)nq * d.nx * 32;               // qe_i [32 nx]
  d.off_r = at;  at += ((int64_t)nq + 3) / 4 * 4;             // re_i
  d.off_C = at;  at += (int64_t)d.Cb * d.kg * 256;            // C, rows
  d.off_CT = at; at += (int64_t)d.Cb * d.nx * 1024;           // C, columns
  d.off_c0 = at; at += (int64_t)d.Cb * 32;                    // c0 [32 Cb]
  d.total = at + 4;                                           // (never empty)
  return d;
}

// dc3_tile_served(): the one rule.  fp32; n in one or two blocks of 32 (what the kernels keep in registers); m, nq and
// no = k - n are bounded only by the image: nothing whose size depends on them is held in LDS or registers.
inline bool dc3_tile_served(const int n, const int m, const int nq, const int no) {
  if (n < 1 || n > kDc3TileMaxN || m < 0 || nq < 0 || no < 0) return false;
  return dc3_tile_dims(n, m, nq, no).total * (int64_t)sizeof(float) <= kDc3TileMaxImageBytes;
}

namespace dc3_tile_detail {

// M(r, c) = src[r * rs + c * cs] inside rows x cols, 0 outside
struct View {
  const double* src;
  int rows, cols;
  int64_t rs, cs;
  float at(const int r, const int c) const {
    return (r < rows && c < cols) ? (float)src[(int64_t)r * rs + (int64_t)c * cs] : 0.0f;
  }
};

inline void lay_rows(const View& M, const int blocks, const int kg, float* out) {
  for (int b = 0; b < blocks; ++b)
    for (int g = 0; g < kg; ++g)
      for (int l = 0; l < 64; ++l) {
        const int r = 32 * b + (l & 31), c = 8 * g + 4 * (l >> 5);
        float* dst = out + (((int64_t)b * kg + g) * 64 + l) * 4;
        for (int e = 0; e < 4; ++e) dst[e] = M.at(r, c + e);
      }
}

inline void lay_columns(const View& M, const int blocks, const int nx, float* out) {
  for (int b = 0; b < blocks; ++b)
    for (int ob = 0; ob < nx; ++ob)
      for (int g = 0; g < 4; ++g)
        for (int l = 0; l < 64; ++l) {
          const int r = 32 * b + 8 * g + 4 * (l >> 5), c = 32 * ob + (l & 31);
          float* dst = out + ((((int64_t)b * nx + ob) * 4 + g) * 64 + l) * 4;
          for (int e = 0; e < 4; ++e) dst[e] = M.at(r + e, c);
        }
}

}  // namespace dc3_tile_detail

// The image of a set (arrays as rayen_dc3_pack_create takes them: fp64, row-major); false where the shape is not served.
inline bool dc3_tile_image(const int n, const int m, const int nq, const int no, const double* A1e, const double* b1e,
                           const double* Pe, const double* qe, const double* re, const double* C, const double* c0,
                           std::vector<float>* out) {
  using dc3_tile_detail::View;
  if (!dc3_tile_served(n, m, nq, no)) return false;
  const Dc3TileDims d = dc3_tile_dims(n, m, nq, no);
  std::vector<float>& h = *out;
  h.assign((size_t)d.total, 0.0f);
  const View A{A1e, m, n, n, 1};
  dc3_tile_detail::lay_rows(A, d.Mb, d.kg, h.data() + d.off_A);
  dc3_tile_detail::lay_columns(A, d.Mb, d.nx, h.data() + d.off_AT);
  for (int i = 0; i < m; ++i) h[(size_t)d.off_b + i] = (float)b1e[i];
  for (int c = 0; c < nq; ++c) {
    const double* P = Pe + (int64_t)c * n * n;
    dc3_tile_detail::lay_rows(View{P, n, n, n, 1}, d.nx, d.kg, h.data() + d.off_P + (int64_t)c * d.nx * d.kg * 256);
    dc3_tile_detail::lay_rows(View{P, n, n, 1, n}, d.nx, d.kg, h.data() + d.off_PT + (int64_t)c * d.nx * d.kg * 256);
    for (int j = 0; j < n; ++j) h[(size_t)(d.off_q + (int64_t)c * d.nx * 32 + j)] = (float)qe[(int64_t)c * n + j];
    h[(size_t)d.off_r + c] = (float)re[c];
  }
  const View Cv{C, no, n, n, 1};
  dc3_tile_detail::lay_rows(Cv, d.Cb, d.kg, h.data() + d.off_C);
  dc3_tile_detail::lay_columns(Cv, d.Cb, d.nx, h.data() + d.off_CT);
  for (int o = 0; o < no; ++o) h[(size_t)d.off_c0 + o] = (float)c0[o];
  return true;
}

}  // namespace rayen
