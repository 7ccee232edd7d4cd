"""The host-only helpers the side layers share (rayen_amd/csrc/rayen_side_layout.h: ``align256``, ``padded_width`` /
``dispatch_width``, the scratch-buffer layouts of DC3 and the projection) against an independent restatement in Python
integers (no GPU).

A small host-only C++ program includes the header and prints the results.  The expected values are computed here: the
padded width as a ternary chain (``k <= 4 ? 4 : ... : 64`` for Bar and DC3, ``k <= 8 ? 8 : ... : 64`` for the soft cost's
fp64 image), the instance a width reaches as a ``switch`` over the powers of two, and every scratch size and region offset
from ``tests/side_layout_formulas.py``.  Exact equality."""
import itertools
import shutil
import subprocess

from rayen_amd import _build

import side_layout_formulas as formulas

ALIGN = [0, 1, 255, 256, 257, 2 ** 32 + 1]
WIDTHS = range(1, 66)
NS, MS, ELEMS = (1, 7, 64), (1, 65, 576), (4, 8)
UNSUPPORTED = -6             # RAYEN_E_UNSUPPORTED (include/rayen_hip.h)


def _chain(w, lo):
    """the ternary chain from ``lo`` to 64; nothing beyond 64 (the callers refuse such a width before they ask)"""
    for K in (4, 8, 16, 32, 64):
        if K >= lo and w <= K:
            return K
    return 0


def _dc3_cases():
    return list(itertools.product(NS, formulas.BATCHES, formulas.STEPS, ELEMS))


def _proj_cases():
    return list(itertools.product(NS, MS, formulas.BATCHES, ELEMS, (0, 1)))


def test_side_layout_helpers_match_the_written_out_formulas(tmp_path):
    src = tmp_path / "side_layout_probe.cpp"
    src.write_text("""
#include <cstdio>
#include "rayen_side_layout.h"
template <int LO, int HI>
static void widths() {
  for (int w = 1; w <= 65; ++w) {
    const int K = rayen::padded_width<LO, HI>(w);
    int seen = 0;
    // the padded width reaches its instance; the raw width reaches one only where it is a power of two in range
    const int rc = rayen::dispatch_width<LO, HI>(K, [&](auto Kc) { seen = Kc(); return 0; });
    int raw = 0;
    const int rc_raw = rayen::dispatch_width<LO, HI>(w, [&](auto Kc) { raw = Kc(); return 0; });
    std::printf("%d %d %d %d %d\\n", K, rc, seen, rc_raw, raw);
  }
}
template <int N>
static void show(const rayen::WsLayout<N>& l) {
  std::printf("%zu", l.total);
  for (int i = 0; i < N; ++i) std::printf(" %zu %zu", l.offset[i], l.bytes[i]);
  std::printf("\\n");
}
int main() {
  const size_t align[] = {@ALIGN@};
  for (const size_t x : align) std::printf("%zu\\n", rayen::align256(x));
  widths<4, 64>();
  widths<8, 64>();
  const int ns[] = {@NS@}, ms[] = {@MS@}, steps[] = {@STEPS@};
  const long long batches[] = {@BATCHES@};
  const size_t elems[] = {@ELEMS@};
  for (const int n : ns)
    for (const long long B : batches)
      for (const int s : steps)
        for (const size_t e : elems) {
          show(rayen::dc3_forward_ws(n, B, s, (s + @CHUNK@ - 1) / @CHUNK@, e));
          show(rayen::dc3_backward_ws(n, B, s, e));
        }
  for (const int n : ns)
    for (const int m : ms)
      for (const long long B : batches)
        for (const size_t e : elems)
          for (int backward = 0; backward < 2; ++backward) show(rayen::proj_ws(n, m, B, backward != 0, e));
  // a region the call does not use has no address; the others sit at their offsets
  alignas(256) static unsigned char buf[4096];
  const rayen::WsLayout<3> l = rayen::proj_ws(3, 5, 7, false, 4);
  std::printf("%d %d %d\\n", (int)(l.at<unsigned char>(buf, rayen::kProjXs) == buf),
              (int)(l.at<unsigned char>(buf, rayen::kProjStatus) == buf + l.offset[1]),
              (int)(l.at<unsigned char>(buf, rayen::kProjDvs) == nullptr));
  std::printf("%zu %zu\\n", rayen::kLdsBudget, rayen::kLdsNoOptIn);
  return 0;
}
""")
    values = dict(ALIGN=", ".join(f"{x}ull" for x in ALIGN), NS=", ".join(map(str, NS)), MS=", ".join(map(str, MS)),
                  STEPS=", ".join(map(str, formulas.STEPS)), BATCHES=", ".join(f"{b}ll" for b in formulas.BATCHES),
                  ELEMS=", ".join(map(str, ELEMS)), CHUNK=str(formulas.DC3_CHUNK))
    text = src.read_text()
    for key, value in values.items():
        text = text.replace(f"@{key}@", value)
    src.write_text(text)
    exe = tmp_path / "side_layout_probe"
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    cmd = [gxx, "-std=c++17", "-Wall", "-Werror", "-I", _build.CSRC, "-I", _build.INCLUDE, str(src), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stderr)
    lines = iter(ran.stdout.strip().splitlines())

    for x in ALIGN:
        assert int(next(lines)) == (x + 255) // 256 * 256, x
    for lo in (4, 8):
        for w in WIDTHS:
            want = _chain(w, lo)
            power = w if (w >= lo and w <= 64 and w & (w - 1) == 0) else 0
            got = [int(t) for t in next(lines).split()]
            assert got == [want, 0 if want else UNSUPPORTED, want, 0 if power else UNSUPPORTED, power], (lo, w, got)
    for n, B, steps, elem in _dc3_cases():
        for total, offsets in (formulas.dc3_forward(n, B, steps, elem), formulas.dc3_backward(n, B, steps, elem)):
            got = [int(t) for t in next(lines).split()]
            assert got[0] == total and got[1::2] == offsets, (n, B, steps, elem, got, total, offsets)
            assert sum(got[2::2]) == total
    for n, m, B, elem, backward in _proj_cases():
        total, offsets = formulas.proj(n, m, B, elem, backward)
        got = [int(t) for t in next(lines).split()]
        assert got[0] == total and got[1::2] == offsets, (n, m, B, elem, backward, got, total, offsets)
        assert (got[6] != 0) == bool(backward and B)
    assert next(lines).split() == ["1", "1", "1"]
    assert next(lines).split() == [str(160 * 1024), str(48 * 1024)]
    assert next(lines, None) is None
