"""The probe constant behind the forward's leading-product probe (rayen_amd/csrc/rayen_tiles.h::pair_probe_constant; the
W-in-LDS walk of rayen_mfma_pair_wl.hip multiplies only the leading f16 pieces a1 b1 of a quadratic / cone first and skips the
segment when (sqrt(sum of squares of those) + sqrt(cabs) ||sv v||)^2 through the segment's closer is below the running
maximum, so that expression must never be below the sum of squares the full three-product walk reaches).  A stand-alone host
program around the helper: the f16-pair split of the rows (as the image does it) and of sv v (as pair_split_* do it, round to
nearest even), the full accumulators (a2 b1, a1 b2 per K-step, then a1 b1 -- the walk's order) and the probe accumulators summed
in fp32, and for each factor  ||full|| <= sqrt(total_probe) + sqrt(cabs) ||sv v||  as well as the kernel's own fp32 expression
against the fp32 sum of squares of the full accumulators, over 10^4 directions per factor shape: random ones, the coordinate axes, and the
Perron vector of |R|'|R| (all signs aligned: it maximises || |R| |x| ||) with and without sign flips.  Factor shapes: dense,
triangular halves like the shared tiles', rank-deficient, badly scaled (f16 subnormals), a single row, all zero.  Reports the
largest share of the margin any direction used.  No GPU."""
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

using rayen::pair_probe_constant;

static const int n = 64;

struct Factor {
  int m;                       // rows, a multiple of 32 (zero rows pad a tile, as in the image)
  std::vector<float> a1, a2;   // the two f16 pieces of every scaled entry, as floats
};

// direction -> how much of the margin it used (<= 1 is the claim); -1: a violation of the kernel's fp32 expression
static double used(const Factor& F, const float cabs, const std::vector<double>& v, bool* fp32_fail) {
  double big = 0.0;
  for (const double x : v) big = std::fmax(big, std::fabs(x));
  if (!(big > 0.0)) return 0.0;
  int ex = 0;
  (void)std::frexp(big, &ex);                       // big = f 2^ex, f in [0.5, 1): sv puts it into [2^13, 2^14)
  const float sv = std::ldexp(1.0f, 14 - ex);
  std::vector<float> x(n), b1(n), b2(n);
  float nv2 = 0.f;
  for (int j = 0; j < n; ++j) {
    x[j] = (float)v[j] * sv;
    const _Float16 h1 = (_Float16)x[j];
    const _Float16 h2 = (_Float16)(x[j] - (float)h1);
    b1[j] = (float)h1;
    b2[j] = (float)h2;
    nv2 = std::fmaf(x[j], x[j], nv2);
  }
  double full2 = 0.0, nx2 = 0.0;
  float tot_probe = 0.f, tot_full = 0.f;
  for (int j = 0; j < n; ++j) nx2 += (double)x[j] * (double)x[j];
  for (int i = 0; i < F.m; ++i) {
    const float* r1 = &F.a1[(size_t)i * n];
    const float* r2 = &F.a2[(size_t)i * n];
    float full = 0.f, probe = 0.f;
    for (int sp = 0; sp < n / 16; ++sp) {
      for (int j = 16 * sp; j < 16 * sp + 16; ++j) full = std::fmaf(r2[j], b1[j], full);
      for (int j = 16 * sp; j < 16 * sp + 16; ++j) full = std::fmaf(r1[j], b2[j], full);
    }
    for (int j = 0; j < n; ++j) full = std::fmaf(r1[j], b1[j], full);
    for (int j = 0; j < n; ++j) probe = std::fmaf(r1[j], b1[j], probe);
    full2 += (double)full * (double)full;
    tot_probe = std::fmaf(probe, probe, tot_probe);
    tot_full = std::fmaf(full, full, tot_full);
  }
  // the kernel's expression, in fp32
  const float r = std::sqrt(std::fmax(tot_probe, 0.f)) + std::sqrt(cabs * nv2);
  const float ub = (r * r) * 1.000244140625f;
  if (!(ub >= tot_full)) *fp32_fail = true;
  const double margin = std::sqrt((double)cabs) * std::sqrt(nx2);
  const double need = std::sqrt(full2) - std::sqrt((double)tot_probe);
  if (!(margin > 0.0)) return need > 0.0 ? 2.0 : 0.0;
  return need / margin;
}

int main() {
  std::mt19937_64 gen(2468);
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  std::normal_distribution<double> nrm(0.0, 1.0);
  int bad = 0, cases = 0;
  double worst = -1e300;
  for (int kind = 0; kind < 7; ++kind)
    for (int rep = 0; rep < 3; ++rep) {
      const int m0 = kind == 4 ? 1 : (kind == 1 ? 64 : 32 + 16 * rep);
      const int m = (m0 + 31) / 32 * 32;
      std::vector<std::vector<double>> R(m, std::vector<double>(n, 0.0));
      for (int i = 0; i < m0; ++i)
        for (int j = 0; j < n; ++j) {
          double x = uni(gen);
          if (kind == 1 && i >= 5) x = 0.0;                                  // rank 5 of 64 rows ...
          if (kind == 2) x = j >= i ? x : 0.0;                               // upper triangular
          if (kind == 3) x = (i < 32 || j < 32) ? x : 0.0;                   // dense rows + rows over one column half
          if (kind == 5) x *= std::ldexp(1.0, (i % 7) * 6 - 36);             // rows over 36 binades: f16 subnormals and zeros
          if (kind == 6) x = 0.0;                                            // all zero
          R[i][j] = x;
        }
      if (kind == 1)
        for (int i = 5; i < m0; ++i)
          for (int j = 0; j < n; ++j) R[i][j] = R[i % 5][j] * (1.0 + i) / 64.0;     // ... the others multiples of the first five
      // gW: the largest entry into [2^13, 2^14), as the image does it
      double big = 0.0;
      for (const auto& r : R) for (const double x : r) big = std::fmax(big, std::fabs(x));
      int ex = 0;
      if (big > 0.0) (void)std::frexp(big, &ex);
      const double gW = big > 0.0 ? std::ldexp(1.0, 14 - ex) : 1.0;
      Factor F;
      F.m = m;
      F.a1.resize((size_t)m * n);
      F.a2.resize((size_t)m * n);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j) {
          const float a = (float)R[i][j] * (float)gW;
          const _Float16 h1 = (_Float16)a;
          const _Float16 h2 = (_Float16)(a - (float)h1);
          F.a1[(size_t)i * n + j] = (float)h1;
          F.a2[(size_t)i * n + j] = (float)h2;
        }
      std::vector<const double*> rows;
      for (const auto& r : R) rows.push_back(r.data());
      const double ca = pair_probe_constant(rows, n, gW);
      float cabs = (float)ca;
      if ((double)cabs < ca) cabs = std::nextafter(cabs, INFINITY);
      ++cases;
      if (kind == 6) {
        if (ca != 0.0) { ++bad; std::printf("zero rows: constant %g\n", ca); }
        continue;
      }
      if (!(cabs > 0.f)) { ++bad; std::printf("kind %d: no constant\n", kind); continue; }
      // the Perron vector of |R|'|R| by power iteration
      std::vector<double> pv(n, 1.0);
      for (int iter = 0; iter < 2000; ++iter) {
        std::vector<double> t(m, 0.0), w(n, 0.0);
        for (int i = 0; i < m; ++i) for (int j = 0; j < n; ++j) t[i] += std::fabs(R[i][j]) * pv[j];
        for (int i = 0; i < m; ++i) for (int j = 0; j < n; ++j) w[j] += std::fabs(R[i][j]) * t[i];
        double nw = 0.0;
        for (const double x : w) nw += x * x;
        nw = std::sqrt(nw);
        if (!(nw > 0.0)) break;
        for (int j = 0; j < n; ++j) pv[j] = w[j] / nw;
      }
      bool fp32_fail = false;
      double top = -1e300;
      for (int d = 0; d < 3400; ++d) {      // (three factors per shape: 10^4 directions per shape)
        std::vector<double> u(n, 0.0);
        if (d < n) u[d] = 1.0;
        else if (d == n) u = pv;
        else if (d < 3 * n) for (int j = 0; j < n; ++j) u[j] = pv[j] * (uni(gen) < 0.0 ? -1.0 : 1.0);      // sign flips
        else if (d < 4 * n) for (int j = 0; j < n; ++j) u[j] = pv[j] * (1.0 + 1e-3 * nrm(gen));            // around it
        else if (d % 3 == 0) for (double& x : u) x = uni(gen);
        else if (d % 3 == 1) for (double& x : u) x = nrm(gen) * std::ldexp(1.0, (int)(uni(gen) * 12));     // entries over 24 binades
        else for (double& x : u) x = nrm(gen);
        const double share = used(F, cabs, u, &fp32_fail);
        top = std::fmax(top, share);
        if (!(share <= 1.0)) { ++bad; std::printf("kind %d rep %d direction %d uses %.6f of the margin\n", kind, rep, d, share); break; }
      }
      if (fp32_fail) { ++bad; std::printf("kind %d rep %d: the kernel's fp32 expression fell below the full sum of squares\n", kind, rep); }
      std::printf("kind %d rep %d: largest share of the margin used %.4f\n", kind, rep, top);
      worst = std::fmax(worst, top);
    }
  std::printf("cases %d bad %d worst share of the margin %.4f\n", cases, bad, worst);
  return bad == 0 ? 0 : 1;
}
"""


def test_the_probe_margin_covers_the_dropped_products(tmp_path):
    src = tmp_path / "probe_bound.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "probe_bound"
    cmd = [_build.hipcc_path(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", _build.INCLUDE,
           "-I", _build.CSRC, str(src), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    print(ran.stdout)
    assert ran.returncode == 0, (ran.stdout, ran.stderr)
    assert "cases 21 bad 0" in ran.stdout
