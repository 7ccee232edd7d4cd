// The operand images of the fp64 DC3 tile kernels (rayen_dc3_tile64.hip) and the rule of what they serve: plain host code
// on host vectors, no HIP call and no HIP type (any C++ compiler takes this header alone).  The fp32 images of
// rayen_dc3_tile_image.h re-cut for v_mfma_f64_16x16x4_f64.
//
// A product of the kernels is  OUT [16 rows x 16 samples] += M_block [16 x K] X [K x 16 samples], four columns of K a
// K-step, with X in accumulator layout (header of rayen_mfma_f64.hip): lane l, register g of a 16-row block of X is sample
// l & 15, row 4 g + (l >> 4).  The B operand of a K-step is B[k = l >> 4][sample = l & 15]: register g of X IS the B operand
// of K-step g of its block, with no permutation of k, and the A operand of that step is M[row l & 15][column 4 g + (l >> 4)].
// An image stores, per lane, the A operands of two consecutive K-steps as one 16-byte pair:
//   rows    [block][gp < kp][lane]          -> M[16 block + (lane & 15)][8 gp + 4 e + (lane >> 4)]            (M X, X of n rows)
//   columns [block][ob < nx][gp < 2][lane]  -> M[16 block + 8 gp + 4 e + (lane >> 4)][16 ob + (lane & 15)]   (M' X, X of 16 rows)
// e = 0, 1; kg = ceil(n / 4) K-steps, kp = ceil(kg / 2) pairs of them, nx = ceil(n / 16); everything outside M is zero.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace rayen {

constexpr int kDc3Tile64MaxN = 64;
constexpr int64_t kDc3Tile64MaxImageBytes = (int64_t)1 << 30;      // the image is one device allocation

struct Dc3Tile64Dims {
  int n = 0, m = 0, nq = 0, no = 0;
  int nx = 0, kg = 0, kp = 0, Mb = 0, Cb = 0;      // blocks of n; K-steps of n; pairs of K-steps; row blocks of A1e; of C
  // offsets in doubles, each a multiple of 2
  int64_t off_A = 0, off_AT = 0, off_b = 0, off_P = 0, off_PT = 0, off_q = 0, off_r = 0, off_C = 0, off_CT = 0, off_c0 = 0,
          total = 0;
};

inline Dc3Tile64Dims dc3_tile64_dims(const int n, const int m, const int nq, const int no) {
  Dc3Tile64Dims d;
  d.n = n; d.m = m; d.nq = nq; d.no = no;
  d.nx = (n + 15) / 16; d.kg = (n + 3) / 4; d.kp = (d.kg + 1) / 2;
  d.Mb = (int)(((int64_t)m + 15) / 16); d.Cb = (int)(((int64_t)no + 15) / 16);
  int64_t at = 0;
  d.off_A = at;  at += (int64_t)d.Mb * d.kp * 128;            // A1e, rows
  d.off_AT = at; at += (int64_t)d.Mb * d.nx * 256;            // A1e, columns
  d.off_b = at;  at += (int64_t)d.Mb * 16;                    // b1e [16 Mb]
  d.off_P = at;  at += (int64_t)nq * d.nx * d.kp * 128;       // Pe_i, rows (of its nx blocks)
  d.off_PT = at; at += (int64_t)nq * d.nx * d.kp * 128;       // Pe_i', rows
  d.off_q = at;  at += (int64_t)nq * d.nx * 16;               // qe_i [16 nx]
  d.off_r = at;  at += ((int64_t)nq + 1) / 2 * 2;             // re_i
  d.off_C = at;  at += (int64_t)d.Cb * d.kp * 128;            // C, rows
  d.off_CT = at; at += (int64_t)d.Cb * d.nx * 256;            // C, columns
  d.off_c0 = at; at += (int64_t)d.Cb * 16;                    // c0 [16 Cb]
  d.total = at + 2;                                           // (never empty)
  return d;
}

// dc3_tile64_served(): the one rule.  fp64; n in one to four blocks of 16 (what the kernels keep in registers); m, nq and
// no = k - n are bounded only by the image: nothing whose size depends on them is held in LDS or registers.
inline bool dc3_tile64_served(const int n, const int m, const int nq, const int no) {
  if (n < 1 || n > kDc3Tile64MaxN || m < 0 || nq < 0 || no < 0) return false;
  return dc3_tile64_dims(n, m, nq, no).total * (int64_t)sizeof(double) <= kDc3Tile64MaxImageBytes;
}

namespace dc3_tile64_detail {

// M(r, c) = src[r * rs + c * cs] inside rows x cols, 0 outside
struct View {
  const double* src;
  int rows, cols;
  int64_t rs, cs;
  double at(const int r, const int c) const {
    return (r < rows && c < cols) ? src[(int64_t)r * rs + (int64_t)c * cs] : 0.0;
  }
};

inline void lay_rows(const View& M, const int blocks, const int kp, double* out) {
  for (int b = 0; b < blocks; ++b)
    for (int gp = 0; gp < kp; ++gp)
      for (int l = 0; l < 64; ++l) {
        const int r = 16 * b + (l & 15), c = 8 * gp + (l >> 4);
        double* dst = out + (((int64_t)b * kp + gp) * 64 + l) * 2;
        for (int e = 0; e < 2; ++e) dst[e] = M.at(r, c + 4 * e);
      }
}

inline void lay_columns(const View& M, const int blocks, const int nx, double* out) {
  for (int b = 0; b < blocks; ++b)
    for (int ob = 0; ob < nx; ++ob)
      for (int gp = 0; gp < 2; ++gp)
        for (int l = 0; l < 64; ++l) {
          const int r = 16 * b + 8 * gp + (l >> 4), c = 16 * ob + (l & 15);
          double* dst = out + ((((int64_t)b * nx + ob) * 2 + gp) * 64 + l) * 2;
          for (int e = 0; e < 2; ++e) dst[e] = M.at(r + 4 * e, c);
        }
}

}  // namespace dc3_tile64_detail

// The image of a set (arrays as rayen_dc3_pack_create takes them: fp64, row-major); false where the shape is not served.
inline bool dc3_tile64_image(const int n, const int m, const int nq, const int no, const double* A1e, const double* b1e,
                             const double* Pe, const double* qe, const double* re, const double* C, const double* c0,
                             std::vector<double>* out) {
  using dc3_tile64_detail::View;
  if (!dc3_tile64_served(n, m, nq, no)) return false;
  const Dc3Tile64Dims d = dc3_tile64_dims(n, m, nq, no);
  std::vector<double>& h = *out;
  h.assign((size_t)d.total, 0.0);
  const View A{A1e, m, n, n, 1};
  dc3_tile64_detail::lay_rows(A, d.Mb, d.kp, h.data() + d.off_A);
  dc3_tile64_detail::lay_columns(A, d.Mb, d.nx, h.data() + d.off_AT);
  for (int i = 0; i < m; ++i) h[(size_t)d.off_b + i] = b1e[i];
  for (int c = 0; c < nq; ++c) {
    const double* P = Pe + (int64_t)c * n * n;
    dc3_tile64_detail::lay_rows(View{P, n, n, n, 1}, d.nx, d.kp, h.data() + d.off_P + (int64_t)c * d.nx * d.kp * 128);
    dc3_tile64_detail::lay_rows(View{P, n, n, 1, n}, d.nx, d.kp, h.data() + d.off_PT + (int64_t)c * d.nx * d.kp * 128);
    for (int j = 0; j < n; ++j) h[(size_t)(d.off_q + (int64_t)c * d.nx * 16 + j)] = qe[(int64_t)c * n + j];
    h[(size_t)d.off_r + c] = re[c];
  }
  const View Cv{C, no, n, n, 1};
  dc3_tile64_detail::lay_rows(Cv, d.Cb, d.kp, h.data() + d.off_C);
  dc3_tile64_detail::lay_columns(Cv, d.Cb, d.nx, h.data() + d.off_CT);
  for (int o = 0; o < no; ++o) h[(size_t)d.off_c0 + o] = c0[o];
  return true;
}

}  // namespace rayen
