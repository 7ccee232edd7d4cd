"""The streamed Bar kernels without a device: the window layout of rayen_amd/csrc/rayen_bar_stream_layout.h against its
Python restatement (tests/bar_stream_cases.py) and against the properties it promises, the binding against the header, and
the module's ``bar_kernel`` keyword on host tensors.

A small host-only C++ program includes the header alone and prints, for every (case, precision, window) of the table, the
window count, the piece-to-window map, both window sequences and the launch geometry; the expectations are computed here."""
import os
import pickle
import re
import shutil
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bar_reference as br                                    # noqa: E402
import bar_stream_cases as S                                  # noqa: E402
from helpers import load_golden                               # noqa: E402
from rayen_amd import _build, _lib, workloads                 # noqa: E402
from rayen_amd.constraint_module import ConstraintModule      # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_probe(tmp_path):
    calls = "\n".join(f"  job({j}, {c.nv}, {c.nv + c.nr}, {br.pad_k(c.k)}, {S.ELEM[d]}, {w}ll);" for j, (c, d, w) in enumerate(S.JOBS))
    src = tmp_path / "bar_stream_probe.cpp"
    src.write_text("""
#include <cstdio>
#include "rayen_bar_stream_layout.h"
using namespace rayen;
static void seq(const char* tag, const BarStreamSeq& s) {
  std::printf("%s", tag);
  for (int i = 0; i < bar_stream_seq_steps(s); ++i) std::printf(" %d", bar_stream_seq_window(s, i));
  std::printf("\\n");
}
static void job(int j, long long nv, long long m, int K, long long elem, long long window) {
  const long long g = bar_stream_groups(window, K, elem);
  const long long lds = bar_stream_lds_bytes(m, g, K, elem);
  std::printf("job %d %lld %lld %lld %lld %lld %lld %d\\n", j, g, (long long)bar_stream_windows(m, g),
              (long long)bar_stream_buffer_bytes(m, g, K, elem), lds, (long long)bar_stream_wg_per_cu(lds),
              (long long)bar_stream_rows_per_pass(m, K, elem == 8), bar_stream_group_log2(m));
  std::printf("map");
  for (long long p = 0; p < bar_stream_pieces(m); ++p) std::printf(" %lld", (long long)bar_stream_window_of(p, g));
  std::printf("\\n");
  seq("fwd", bar_stream_forward_seq(nv, m, g));
  seq("bwd", bar_stream_backward_seq(nv, m, g));
}
int main() {
  std::printf("consts %lld %lld %lld %d\\n", (long long)kBarStreamWindow, (long long)kBarStreamMaxWindow,
              (long long)kBarStreamYpBytes, kBarStreamThreads);
  std::printf("ok %d %d %d %d %d %d %d\\n", (int)bar_stream_window_ok(0), (int)bar_stream_window_ok(16),
              (int)bar_stream_window_ok(24), (int)bar_stream_window_ok(-16), (int)bar_stream_window_ok(kBarStreamWindow),
              (int)bar_stream_window_ok(kBarStreamWindow + 16), (int)bar_stream_window_ok(kBarStreamWindow - 16));
  std::printf("groups %lld %lld %lld\\n", (long long)bar_stream_groups(48, 4, 4), (long long)bar_stream_groups(64, 4, 4),
              (long long)bar_stream_groups(0, 16, 4));
  std::printf("rows");
  for (int f64 = 0; f64 < 2; ++f64)
    for (int K = 4; K <= 64; K *= 2) std::printf(" %d", bar_stream_rows(K, f64));
  std::printf("\\n");
""" + calls + "\n  return 0;\n}\n")
    exe = tmp_path / "bar_stream_probe"
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    built = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", _build.CSRC, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stderr)
    return ran.stdout.strip().splitlines()


def test_layout_matches_the_restatement_and_keeps_its_promises(tmp_path):
    lines = _run_probe(tmp_path)
    assert lines[0].split() == ["consts", str(S.DEFAULT_WINDOW), str(S.MAX_WINDOW), str(S.YP_BYTES), str(S.THREADS)]
    assert S.DEFAULT_WINDOW <= S.MAX_WINDOW and 2 * S.MAX_WINDOW + S.YP_BYTES <= br.LDS_BUDGET and S.THREADS == br.THREADS
    # window_ok at its edges: 0, 16, not a multiple of 16, negative, the default, one piece past it, one piece short of it
    assert lines[1].split() == ["ok", "1", "1", "0", "0", "1", "0", "1"]
    assert [S.window_ok(w) for w in (0, 16, 24, -16, S.DEFAULT_WINDOW, S.DEFAULT_WINDOW + 16, S.DEFAULT_WINDOW - 16)] == \
        [True, True, False, False, True, False, True]
    # a window below one group of four generators holds zero groups (the library's RAYEN_E_BAD_ARG); 0 is the default
    assert lines[2].split() == ["groups", "0", "1", str(S.DEFAULT_WINDOW // 256)]
    assert (S.groups(48, 4, 4), S.groups(64, 4, 4), S.groups(0, 16, 4)) == (0, 1, S.DEFAULT_WINDOW // 256)
    assert lines[3].split()[1:] == [str(S.rows(K, f64)) for f64 in (0, 1) for K in (4, 8, 16, 32, 64)]
    body = lines[4:]
    assert len(body) == 4 * len(S.JOBS)
    mixed_next_to_a_cut = overlap = second_run_elsewhere = 0
    for j, (case, dtype_name, window) in enumerate(S.JOBS):
        what = f"{case.name} {dtype_name} window {window}"
        head, pmap, fwd, bwd = (line.split() for line in body[4 * j:4 * j + 4])
        K, elem, nv, m = br.pad_k(case.k), S.ELEM[dtype_name], case.nv, case.nv + case.nr
        g = S.groups(window, K, elem)
        lds = S.lds_bytes(m, g, K, elem)
        assert head == ["job", str(j), str(g), str(S.windows(m, g)), str(S.buffer_bytes(m, g, K, elem)), str(lds),
                        str(S.wg_per_cu(lds)), str(S.rows_per_pass(m, K, elem == 8)), str(S.group_log2(m))], what
        assert (pmap[0], fwd[0], bwd[0]) == ("map", "fwd", "bwd")
        pmap, fwd, bwd = ([int(x) for x in f[1:]] for f in (pmap, fwd, bwd))
        assert pmap == [S.window_of(p, g) for p in range(S.pieces(m))] and fwd == S.forward_seq(nv, m, g) \
            and bwd == S.backward_seq(nv, m, g), what
        # the restated geometry is the resident kernels'
        assert 1 << S.group_log2(m) == br.lanes(m) and S.rows_per_pass(m, K, elem == 8) == br.rows_per_iter(m) * S.rows(K, elem == 8)
        # windows are whole groups of four, within the window size, and everything fits LDS
        nw = S.windows(m, g)
        assert g >= 1 and g * 4 * K * elem <= (window or S.DEFAULT_WINDOW) and lds <= br.LDS_BUDGET, what
        assert S.buffer_bytes(m, g, K, elem) % (4 * K * elem) == 0 and S.buffer_bytes(m, g, K, elem) % 16 == 0, what
        # every piece is in exactly one window; the windows are 0 .. nw - 1 in order, g pieces each but the last
        assert len(pmap) == S.pieces(m) and pmap == sorted(pmap) and set(pmap) == set(range(nw)), what
        assert all(pmap.count(w) == g for w in range(nw - 1)) and 1 <= pmap.count(nw - 1) <= g, what
        # forward: the windows of the vertex pieces, then those of the ray pieces, each run ascending and without a gap
        pv, pr = S.pieces(nv), nv // 4
        first = sorted({pmap[p] for p in range(pv)})
        second = sorted({pmap[p] for p in range(pr, S.pieces(m))}) if case.nr else []
        assert fwd == first + second, what
        assert bwd == first + list(range(nw)), what
        for run in (first, second):
            assert run == list(range(run[0], run[0] + len(run))) if run else True, what
        assert set(fwd) == set(range(nw)) and len(fwd) >= 1, what
        overlap += bool(first and second and first[-1] == second[0])
        second_run_elsewhere += bool(first and second and first[-1] != second[0])
        mixed_next_to_a_cut += bool(nv % 4 and case.nr and nw > 1 and (pr % g in (0, g - 1)))
        # what a pass copies: never more than its steps, exactly one window where the set is one
        assert S.copies(fwd) <= len(fwd) and S.copies(fwd, 2) <= 2 * len(fwd)
        if nw == 1:
            assert S.copies(fwd, 3) == 1 and S.copies(bwd, 3) == 1, what
    assert overlap and second_run_elsewhere and mixed_next_to_a_cut          # the cases reach every branch


def test_binding_and_header_declare_the_same_entry_points():
    text = open(os.path.join(REPO, "include", "rayen_hip_bar_stream.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.EXPORTS_BAR_STREAM)
    assert not set(declared) & set(_lib.EXPORTS)
    assert '#include "rayen_hip_bar_stream.h"' in open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    # argument checks that need no device
    assert lib.rayen_bar_resident_served(None, 0) == 0
    assert lib.rayen_bar_stream_forward_f32(None, None, 0, 1, None, 1, None, None, 0, None) == -1
    assert lib.rayen_bar_stream_forward_f64(None, None, 0, 1, None, 1, None, None, 0, None) == -1
    assert lib.rayen_bar_stream_backward_f32(None, None, 1, None, None, 0, None, 0, None) == -1
    assert lib.rayen_bar_stream_backward_f64(None, None, 1, None, None, 0, None, 0, None) == -1


def _cs():
    return workloads.build_constraints(load_golden("example_08")[0])


def _q(layer, dtype=torch.float32):
    gen = torch.Generator().manual_seed(3)
    return torch.empty(37, layer.getDimAfterMap(), 1, dtype=dtype).uniform_(-3, 3, generator=gen)


@pytest.mark.parametrize("kernel", ["resident", "stream", "auto"])
def test_host_tensors_take_the_reference_formula_under_every_kernel(kernel):
    layer = ConstraintModule(_cs(), method="Bar", create_map=False, bar_kernel=kernel)
    assert layer.bar_kernel == kernel and layer._route_key() == (False if kernel == "resident" else kernel)
    for dtype in (torch.float32, torch.float64):
        q = _q(layer, dtype).requires_grad_(True)
        want = layer._bar_reference(q.detach())
        y = layer(q)
        assert torch.equal(y, want)
        y.sum().backward()
        assert q.grad is not None and torch.isfinite(q.grad).all()


def test_unknown_values_and_other_methods_are_value_errors():
    cs = _cs()
    with pytest.raises(ValueError):
        ConstraintModule(cs, method="Bar", create_map=False, bar_kernel="bogus")
    for kernel in ("stream", "auto"):
        with pytest.raises(ValueError):
            ConstraintModule(cs, method="RAYEN", create_map=False, bar_kernel=kernel)
    assert ConstraintModule(cs, method="RAYEN", create_map=False, bar_kernel="resident").bar_kernel == "resident"
    for bad in (-16, 24, 1.5, True):
        with pytest.raises(ValueError):
            ConstraintModule(cs, method="Bar", create_map=False, bar_kernel="stream", bar_window_bytes=bad)
    with pytest.raises(ValueError):
        ConstraintModule(cs, method="Bar", create_map=False, bar_window_bytes=4096)          # (the resident kernel has no window)
    with pytest.raises(TypeError):
        ConstraintModule(cs, None, "Bar", False, None, "stream")          # keyword-only: the positional signature stays


@pytest.mark.parametrize("kernel", ["resident", "stream", "auto"])
def test_pickle_round_trips_keep_the_choice(kernel):
    layer = ConstraintModule(_cs(), method="Bar", create_map=False, bar_kernel=kernel,
                             bar_window_bytes=0 if kernel == "resident" else 4096)
    assert layer.bar_window_bytes == (0 if kernel == "resident" else 4096)
    again = pickle.loads(pickle.dumps(layer))
    assert again.bar_kernel == kernel and again.bar_window_bytes == layer.bar_window_bytes
    q = _q(layer)
    assert torch.equal(again(q), layer(q))


def test_a_pickle_from_before_the_keyword_loads_as_resident():
    layer = ConstraintModule(_cs(), method="Bar", create_map=False)
    state = layer.__getstate__()
    del state["bar_kernel"], state["bar_window_bytes"]
    old = ConstraintModule.__new__(ConstraintModule)
    old.__setstate__(state)
    assert old.bar_kernel == "resident" and old.bar_window_bytes == 0 and old._route_key() is False
    q = _q(layer)
    assert torch.equal(old(q), layer(q))
