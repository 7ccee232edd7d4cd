// The operand images of the DC3 tile kernels (rayen_dc3_tile_kernel.h) and the rule of what they serve, once for both
// geometries: plain host code on host vectors, no HIP call and no HIP type (any C++ compiler takes this header alone).
//
// A product of the kernels is  OUT [R rows x R samples] += M_block [R x K] X [K x R samples]  on the matrix cores, with X in
// accumulator layout: lane l, register i of an R-row block of X is sample l % R, row row_of(i, l / R).  The B operand of a
// K-step is B[k = l / R][sample = l % R]: register i of X IS the B operand of one K-step, and the A operand of that step is
// M[row l % R][column row_of(i, l / R)].  An image stores, per lane, the A operands of E consecutive registers as one 16-byte
// pack; a pack covers 8 columns in both geometries (E registers in each of the 64 / R lane groups):
//   rows    [block][g < kp][lane]              -> M[R block + lane % R][8 g + row_of(e, lane / R)]            (M X, X of n rows)
//   columns [block][ob < nx][g < R / 8][lane]  -> M[R block + 8 g + row_of(e, lane / R)][R ob + lane % R]     (M' X, X of R rows)
// e < E, kp = ceil(n / 8), nx = ceil(n / R); everything outside M is zero.
//
//                     Dc3TileLayout32 (v_mfma_f32_32x32x2_f32)      Dc3TileLayout64 (v_mfma_f64_16x16x4_f64)
//   R, E              32, 4 (a float4: four K-steps)                16, 2 (two doubles: two K-steps)
//   row_of(i, grp)    8 (i >> 2) + 4 grp + (i & 3)                  4 i + grp
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace rayen {

constexpr int kDc3TileMaxN = 64;
constexpr int64_t kDc3TileMaxImageBytes = (int64_t)1 << 30;      // the image is one device allocation

struct Dc3TileDims {
  int n = 0, m = 0, nq = 0, no = 0;
  int nx = 0, kp = 0, Mb = 0, Cb = 0;      // blocks of n; packs along n (8 columns each); row blocks of A1e; row blocks of C
  // offsets in elements, each a multiple of a pack
  int64_t off_A = 0, off_AT = 0, off_b = 0, off_P = 0, off_PT = 0, off_q = 0, off_r = 0, off_C = 0, off_CT = 0, off_c0 = 0,
          total = 0;
};

// T: the element; ROWS: rows of a block = samples of a tile; PACK: elements of a pack
template <typename T, int ROWS, int PACK>
struct Dc3TileLayout {
  static_assert((ROWS == 32 || ROWS == 16) && 64 % ROWS == 0 && PACK * (64 / ROWS) == 8, "a pack covers 8 columns");
  static constexpr int kRows = ROWS, kPack = PACK;
  static constexpr int kRowsPack = 64 * PACK;                    // elements of one pack of every lane
  static constexpr int kColumnsBlock = ROWS / 8 * kRowsPack;     // elements of a ROWS x ROWS block of a columns image

  // the row of register i of a block in lane group grp: the accumulator layout of the MFMA
  static constexpr int row_of(const int i, const int grp) {
    if constexpr (ROWS == 32) return 8 * (i >> 2) + 4 * grp + (i & 3);
    else return 4 * i + grp;
  }

  static Dc3TileDims dims(const int n, const int m, const int nq, const int no) {
    Dc3TileDims d;
    d.n = n; d.m = m; d.nq = nq; d.no = no;
    d.nx = (n + ROWS - 1) / ROWS; d.kp = (n + 7) / 8;
    d.Mb = (int)(((int64_t)m + ROWS - 1) / ROWS); d.Cb = (int)(((int64_t)no + ROWS - 1) / ROWS);
    int64_t at = 0;
    d.off_A = at;  at += (int64_t)d.Mb * d.kp * kRowsPack;            // A1e, rows
    d.off_AT = at; at += (int64_t)d.Mb * d.nx * kColumnsBlock;        // A1e, columns
    d.off_b = at;  at += (int64_t)d.Mb * ROWS;                        // b1e [ROWS Mb]
    d.off_P = at;  at += (int64_t)nq * d.nx * d.kp * kRowsPack;       // Pe_i, rows (of its nx blocks)
    d.off_PT = at; at += (int64_t)nq * d.nx * d.kp * kRowsPack;       // Pe_i', rows
    d.off_q = at;  at += (int64_t)nq * d.nx * ROWS;                   // qe_i [ROWS nx]
    d.off_r = at;  at += ((int64_t)nq + PACK - 1) / PACK * PACK;      // re_i
    d.off_C = at;  at += (int64_t)d.Cb * d.kp * kRowsPack;            // C, rows
    d.off_CT = at; at += (int64_t)d.Cb * d.nx * kColumnsBlock;        // C, columns
    d.off_c0 = at; at += (int64_t)d.Cb * ROWS;                        // c0 [ROWS Cb]
    d.total = at + PACK;                                              // (never empty)
    return d;
  }

  // served(): the one rule.  n in whole blocks of ROWS up to 64 (what the kernels keep in registers); m, nq and no = k - n
  // are bounded only by the image: nothing whose size depends on them is held in LDS or registers.
  static bool served(const int n, const int m, const int nq, const int no) {
    if (n < 1 || n > kDc3TileMaxN || m < 0 || nq < 0 || no < 0) return false;
    return dims(n, m, nq, no).total * (int64_t)sizeof(T) <= kDc3TileMaxImageBytes;
  }

  // M(r, c) = src[r * rs + c * cs] inside rows x cols, 0 outside
  struct View {
    const double* src;
    int rows, cols;
    int64_t rs, cs;
    T at(const int r, const int c) const { return (r < rows && c < cols) ? (T)src[(int64_t)r * rs + (int64_t)c * cs] : T(0); }
  };

  static void lay_rows(const View& M, const int blocks, const int kp, T* out) {
    for (int b = 0; b < blocks; ++b)
      for (int g = 0; g < kp; ++g)
        for (int l = 0; l < 64; ++l) {
          T* dst = out + (((int64_t)b * kp + g) * 64 + l) * PACK;
          for (int e = 0; e < PACK; ++e) dst[e] = M.at(ROWS * b + l % ROWS, 8 * g + row_of(e, l / ROWS));
        }
  }

  static void lay_columns(const View& M, const int blocks, const int nx, T* out) {
    for (int b = 0; b < blocks; ++b)
      for (int ob = 0; ob < nx; ++ob)
        for (int g = 0; g < ROWS / 8; ++g)
          for (int l = 0; l < 64; ++l) {
            T* dst = out + ((((int64_t)b * nx + ob) * (ROWS / 8) + g) * 64 + l) * PACK;
            for (int e = 0; e < PACK; ++e) dst[e] = M.at(ROWS * b + 8 * g + row_of(e, l / ROWS), ROWS * ob + l % ROWS);
          }
  }

  // The image of a set (arrays as rayen_dc3_pack_create takes them: fp64, row-major); false where the shape is not served.
  static bool image(const int n, const int m, const int nq, const int no, const double* A1e, const double* b1e,
                    const double* Pe, const double* qe, const double* re, const double* C, const double* c0,
                    std::vector<T>* out) {
    if (!served(n, m, nq, no)) return false;
    const Dc3TileDims d = dims(n, m, nq, no);
    std::vector<T>& h = *out;
    h.assign((size_t)d.total, T(0));
    const View A{A1e, m, n, n, 1};
    lay_rows(A, d.Mb, d.kp, h.data() + d.off_A);
    lay_columns(A, d.Mb, d.nx, h.data() + d.off_AT);
    for (int i = 0; i < m; ++i) h[(size_t)d.off_b + i] = (T)b1e[i];
    const int64_t quad = (int64_t)d.nx * d.kp * kRowsPack;
    for (int c = 0; c < nq; ++c) {
      const double* P = Pe + (int64_t)c * n * n;
      lay_rows(View{P, n, n, n, 1}, d.nx, d.kp, h.data() + d.off_P + c * quad);
      lay_rows(View{P, n, n, 1, n}, d.nx, d.kp, h.data() + d.off_PT + c * quad);
      for (int j = 0; j < n; ++j) h[(size_t)(d.off_q + (int64_t)c * d.nx * ROWS + j)] = (T)qe[(int64_t)c * n + j];
      h[(size_t)d.off_r + c] = (T)re[c];
    }
    const View Cv{C, no, n, n, 1};
    lay_rows(Cv, d.Cb, d.kp, h.data() + d.off_C);
    lay_columns(Cv, d.Cb, d.nx, h.data() + d.off_CT);
    for (int o = 0; o < no; ++o) h[(size_t)d.off_c0 + o] = (T)c0[o];
    return true;
  }
};

using Dc3TileLayout32 = Dc3TileLayout<float, 32, 4>;
using Dc3TileLayout64 = Dc3TileLayout<double, 16, 2>;

}  // namespace rayen
