"""The spectral constant behind the forward's screening (rayen_amd/csrc/rayen_tiles.h::spectral_bound_rows; the walk skips a
quadratic / cone when `constant x ||v||^2` through the segment's closer is below the running maximum, so the constant must
never be below ||R v||^2 / ||v||^2).  A stand-alone host program around the helper: random factors of several shapes
(dense, rank-deficient, triangular halves like the shared tiles', badly scaled, a single row, all zero), and for each the
constant against ||R v||^2 / ||v||^2 on 10^4 directions -- random ones, coordinate axes, and the top eigenvector (power
iteration to convergence), where the bound is tight: it must hold there and be within 1e-5 of it.  No GPU."""
import os
import subprocess

from rayen_amd import _build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cmath>
#include <random>
#include <vector>
#include "rayen_tiles.h"

using rayen::spectral_bound_rows;

static double ratio(const std::vector<std::vector<double>>& R, const std::vector<double>& v) {
  double num = 0.0, den = 0.0;
  for (const auto& r : R) {
    double d = 0.0;
    for (size_t j = 0; j < v.size(); ++j) d += r[j] * v[j];
    num += d * d;
  }
  for (const double x : v) den += x * x;
  return den > 0.0 ? num / den : 0.0;
}

int main() {
  std::mt19937_64 gen(12345);
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  std::normal_distribution<double> nrm(0.0, 1.0);
  const int n = 64;
  int bad = 0, cases = 0;
  double worst_slack = 0.0;
  for (int kind = 0; kind < 7; ++kind)
    for (int rep = 0; rep < 3; ++rep) {
      int m = kind == 4 ? 1 : (kind == 1 ? 64 : 32 + 16 * rep);
      std::vector<std::vector<double>> R(m, std::vector<double>(n, 0.0));
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j) {
          double x = uni(gen);
          if (kind == 1 && i >= 5) x = 0.0;                                  // rank 5 of 64 rows ...
          if (kind == 2) x = j >= i ? x : 0.0;                               // upper triangular
          if (kind == 3) x = (i < 32 || j < 32) ? x : 0.0;                   // dense rows + rows over one column half
          if (kind == 5) x *= std::ldexp(1.0, (i % 7) * 6 - 20);             // rows over 36 binades
          if (kind == 6) x = 0.0;                                            // all zero
          R[i][j] = x;
        }
      if (kind == 1)
        for (int i = 5; i < m; ++i)
          for (int j = 0; j < n; ++j) R[i][j] = R[i % 5][j] * (1.0 + i);     // ... the others multiples of the first five
      std::vector<const double*> rows;
      for (const auto& r : R) rows.push_back(r.data());
      const double c = spectral_bound_rows(rows, n);
      ++cases;
      if (kind == 6) { if (c != 0.0) { ++bad; std::printf("zero rows: %g\n", c); } continue; }
      // the top eigenvector by power iteration on R'R
      std::vector<double> v(n);
      for (double& x : v) x = nrm(gen);
      double lam = 0.0;
      for (int iter = 0; iter < 20000; ++iter) {
        std::vector<double> t(m, 0.0), w(n, 0.0);
        for (int i = 0; i < m; ++i) for (int j = 0; j < n; ++j) t[i] += R[i][j] * v[j];
        for (int i = 0; i < m; ++i) for (int j = 0; j < n; ++j) w[j] += R[i][j] * t[i];
        double nw = 0.0;
        for (const double x : w) nw += x * x;
        nw = std::sqrt(nw);
        for (int j = 0; j < n; ++j) v[j] = w[j] / nw;
        if (std::fabs(nw - lam) <= 1e-15 * nw) { lam = nw; break; }
        lam = nw;
      }
      const double top = ratio(R, v);
      if (!(c >= top)) { ++bad; std::printf("kind %d: constant %.17g below the top eigenvector's %.17g\n", kind, c, top); }
      if (!(c <= top * (1.0 + 1e-5))) { ++bad; std::printf("kind %d: constant %.17g loose against %.17g\n", kind, c, top); }
      worst_slack = std::fmax(worst_slack, c / top - 1.0);
      for (int d = 0; d < 10000; ++d) {
        std::vector<double> u(n, 0.0);
        if (d < n) u[d] = 1.0;
        else if (d < 2 * n) for (int j = 0; j < n; ++j) u[j] = v[j] + 1e-3 * nrm(gen);      // around the top eigenvector
        else for (double& x : u) x = nrm(gen);
        if (!(c >= ratio(R, u))) { ++bad; std::printf("kind %d direction %d above the constant\n", kind, d); break; }
      }
    }
  std::printf("cases %d bad %d worst slack %.3g\n", cases, bad, worst_slack);
  return bad == 0 ? 0 : 1;
}
"""


def test_the_constant_bounds_every_direction_and_is_tight_at_the_top_eigenvector(tmp_path):
    src = tmp_path / "screen_bound.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "screen_bound"
    cmd = [_build.hipcc_path(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-I", _build.INCLUDE, "-I", _build.CSRC,
           str(src), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    print(ran.stdout)
    assert ran.returncode == 0, (ran.stdout, ran.stderr)
    assert "cases 21 bad 0" in ran.stdout
