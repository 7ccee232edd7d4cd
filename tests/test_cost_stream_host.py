"""The streamed soft cost without a device: the window partition of rayen_amd/csrc/rayen_cost_stream_layout.h against its
Python restatement (tests/cost_stream_cases.py) and against the properties it promises, the binding against the header, and
the module's ``kernel`` keyword on host tensors.

A small host-only C++ program includes the header alone, cuts every set of the streamed GPU tests at the three forced
window sizes of each precision and prints windows and pieces; the expectations are computed here."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cost_cases                                             # noqa: E402
import cost_stream_cases as S                                 # noqa: E402
import cost_sweep_cases as sweep                              # noqa: E402
from rayen_amd import _build, _lib                            # noqa: E402
from rayen_amd.cost_computer import CostComputer              # noqa: E402
from rayen_amd.soft_cost import SoftCost                      # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sets():
    """name -> arrays: every set beyond the resident envelope, the row-tile sets, and the LMI set's rows."""
    out = {name: S.beyond_case(name).arrays for name in S.BEYOND}
    out.update({f"tile_{n}": sweep.tile_set(n) for n in sweep.TILE_SETS})
    out["lin700_lmi20"] = S.lmi_case().rows_arrays
    return out


def _jobs():
    """(name, dtype, window, items, K) of every cut the probe makes; window is what the header is handed (never 0)."""
    for name, a in _sets().items():
        for dtype_name in S.DTYPES:
            its = S.items(a, dtype_name)
            for window in S.forced_windows(a, dtype_name):
                yield name, dtype_name, window or S.DEFAULT_WINDOW, its, sweep.lane64_K(a["k"])
            yield name, dtype_name, S.smallest_window(a, dtype_name) - 16, its, sweep.lane64_K(a["k"])


def _run_probe(tmp_path, jobs):
    blocks = []
    for j, (_, dtype_name, window, its, K) in enumerate(jobs):
        rows = ", ".join(f"{{{u}, {f}, {s}}}" for u, f, s in its)
        blocks.append(f"  {{ static const rayen::CostStreamItem items[] = {{{rows}}};\n"
                      f"    cut({j}, items, {len(its)}, {int(dtype_name == 'float64')}, {K}, {window}ll); }}")
    src = tmp_path / "stream_probe.cpp"
    src.write_text("""
#include <cstdio>
#include <vector>
#include "rayen_cost_stream_layout.h"
static void cut(int job, const rayen::CostStreamItem* items, long long n, int f64, int K, long long window) {
  int64_t np = 0, total = 0;
  const int64_t nw = rayen::cost_stream_partition(items, n, f64, K, window, nullptr, 0, nullptr, 0, &np, &total);
  std::printf("job %d %lld %lld %lld\\n", job, (long long)nw, (long long)(nw < 0 ? 0 : np), (long long)(nw < 0 ? 0 : total));
  if (nw < 0) return;
  std::vector<rayen::CostStreamWindow> w((size_t)nw);
  std::vector<rayen::CostStreamPiece> p((size_t)np);
  if (rayen::cost_stream_partition(items, n, f64, K, window, w.data(), nw, p.data(), np, nullptr, nullptr) != nw) std::printf("DRIFT\\n");
  for (const auto& x : w) {
    std::printf("w %d %d %d %d %lld :", x.piece0, x.pieces, x.units, x.forms, (long long)x.bytes);
    for (int i = 0; i < x.pieces; ++i) std::printf(" %d,%d,%d", p[x.piece0 + i].item, p[x.piece0 + i].unit0, p[x.piece0 + i].units);
    std::printf("\\n");
  }
}
int main() {
  std::printf("consts %lld %lld %lld %d %d %d %d\\n", (long long)rayen::kCostStreamWindow, (long long)rayen::kCostStreamMinWindow32,
              (long long)rayen::kCostStreamMaxImage, (int)rayen::cost_stream_window_ok(0), (int)rayen::cost_stream_window_ok(24),
              (int)rayen::cost_stream_window_ok(rayen::kCostStreamWindow + 16), (int)rayen::cost_stream_window_ok(-16));
""" + "\n".join(blocks) + "\n  return 0;\n}\n")
    exe = tmp_path / "stream_probe"
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    built = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", _build.CSRC, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stderr)
    assert "DRIFT" not in ran.stdout
    lines = ran.stdout.strip().splitlines()
    assert lines[0].split() == ["consts", str(S.DEFAULT_WINDOW), str(S.MIN_WINDOW32), str(1 << 30), "1", "0", "0", "0"]
    got, cur = {}, None
    for line in lines[1:]:
        f = line.split()
        if f[0] == "job":
            cur = got[int(f[1])] = dict(nw=int(f[2]), np=int(f[3]), total=int(f[4]), windows=[])
        else:
            pieces = [tuple(int(x) for x in piece.split(",")) for piece in f[7:]]
            cur["windows"].append(dict(piece0=int(f[1]), pieces=pieces, units=int(f[3]), forms=int(f[4]), bytes=int(f[5])))
            assert int(f[2]) == len(pieces)
    return got


def test_partition_matches_the_restatement_and_keeps_its_promises(tmp_path):
    jobs = list(_jobs())
    got = _run_probe(tmp_path, jobs)
    assert len(got) == len(jobs)
    split_somewhere = partial_somewhere = refused = 0
    for j, (name, dtype_name, window, its, K) in enumerate(jobs):
        what = f"{name} {dtype_name} window {window}"
        want = S.partition(its, dtype_name, K, window)
        g = got[j]
        if want is None:
            assert g["nw"] == -1, what
            refused += 1
            continue
        assert g["nw"] == len(want) == len(g["windows"]), what
        assert [w["pieces"] for w in g["windows"]] == want, what
        # every unit exactly once and in the stacked order; no quadratic or cone split; every window within its limit
        flat = [p for w in g["windows"] for p in w["pieces"]]
        assert g["np"] == len(flat), what
        at = {}
        order = []
        for item, unit0, units in flat:
            assert units > 0 and unit0 == at.get(item, 0), what
            at[item] = unit0 + units
            if not its[item][2]:
                assert (unit0, units) == (0, its[item][0]), what + ": an item was split"
            order.append(item)
        assert order == sorted(order) and at == {i: it[0] for i, it in enumerate(its)}, what
        piece0 = 0
        for w in g["windows"]:
            assert w["piece0"] == piece0 and w["units"] == sum(n for _, _, n in w["pieces"]), what
            assert w["forms"] == sum(its[i][1] for i, _, _ in w["pieces"]), what
            assert w["bytes"] == S.window_bytes_of(w["pieces"], its, dtype_name, K) <= window and w["bytes"] % 16 == 0, what
            piece0 += len(w["pieces"])
        assert g["total"] == sum(w["bytes"] for w in g["windows"]), what
        # greedy: a window closes only when the next unit (or whole item) does not fit
        for w, nxt in zip(g["windows"], g["windows"][1:]):
            item, unit0, units = nxt["pieces"][0]
            more = 1 if its[item][2] else its[item][0]
            grown = w["pieces"] + [(item, unit0, more)]
            if its[item][2] and w["pieces"][-1][0] == item:          # the same run goes on: no further piece
                grown = w["pieces"][:-1] + [(item, w["pieces"][-1][1], w["pieces"][-1][2] + 1)]
            assert S.window_bytes_of(grown, its, dtype_name, K) > window, what + ": a window closed early without need"
            partial_somewhere += window - w["bytes"] >= (8 * (K + 1) if dtype_name == "float64" else S.TILE_BYTES32)
        split_somewhere += any(its[i][2] and (u0, n) != (0, its[i][0]) for i, u0, n in flat)
    assert split_somewhere and partial_somewhere and refused          # the cases reach every branch


def test_an_item_larger_than_the_window_leaves_the_set_unserved():
    """Of the Python RESTATEMENT alone (``cost_stream_cases.stream_served_by_formula``, which the GPU tests hold the library's
    answers to): the envelope it states.  The header's own refusal (-1) is covered by the ``smallest - 16`` cuts of
    test_partition_matches_the_restatement_and_keeps_its_promises, and the library's by
    tests/test_gpu_soft_cost_stream.py::test_stream_set_argument_checks_and_refusals."""
    a = S.corridor_set()
    for dtype_name in S.DTYPES:
        small = S.smallest_window(a, dtype_name)
        assert S.stream_served_by_formula(a, dtype_name, small) and S.stream_served_by_formula(a, dtype_name)
        assert not S.stream_served_by_formula(a, dtype_name, small - 16)
    # a linear-only set is served down to one tile (fp32) / one row (fp64)
    lin = sweep.tile_set("lin_only")
    assert S.stream_served_by_formula(lin, "float32", S.TILE_BYTES32) and not S.stream_served_by_formula(lin, "float32", S.TILE_BYTES32 - 16)
    one_row = S.bytes64(1, 0, 1, 16)
    assert S.stream_served_by_formula(lin, "float64", one_row) and not S.stream_served_by_formula(lin, "float64", one_row - 16)
    # outside the envelope whatever the window
    assert not S.stream_served_by_formula(sweep.k65_case().arrays, "float32") and not S.stream_served_by_formula(sweep.k65_case().arrays, "float64")
    assert not S.stream_served_by_formula(sweep.tile_set("cone65"), "float32") and S.stream_served_by_formula(sweep.tile_set("cone65"), "float64")


def test_the_sets_beyond_the_resident_envelope_are_beyond_it():
    """Of the CASES, not of the C++ code: by the formulas (``served_by_formula`` of the resident kernels, the restatement of
    the streamed envelope) every set of the GPU tests' second part is over the resident limit and within the streamed one at
    every forced window.  The GPU tests ask the library the same questions."""
    for name, dtype_name in S.BEYOND_PARAMS:
        a = S.beyond_case(name).arrays
        assert not sweep.served_by_formula(a, dtype_name), (name, dtype_name)
        assert S.stream_served_by_formula(a, dtype_name), (name, dtype_name)
        assert all(S.stream_served_by_formula(a, dtype_name, w) for w in S.forced_windows(a, dtype_name)), (name, dtype_name)
    assert not sweep.served_by_formula(S.lmi_case().rows_arrays, "float32")
    c5 = S.c5_shape_case().arrays
    assert (c5["k"], c5["b1"].size, c5["r"].size, c5["b2"].size) == (45, 1050, 72, 15)
    assert len(S.partition(S.items(c5, "float32"), "float32", 64, S.DEFAULT_WINDOW)) > 1


def test_binding_and_header_declare_the_same_entry_points():
    text = open(os.path.join(REPO, "include", "rayen_hip_cost_stream.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.EXPORTS_COST_STREAM)
    assert '#include "rayen_hip_cost_stream.h"' in open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    # argument checks that need no device
    assert lib.rayen_cost_stream_set(None, 0) == -1 and lib.rayen_cost_stream_served(None, 0) == 0
    assert lib.rayen_soft_cost_stream_f32(None, None, 0, 1, None, None, None, None, 0, None) == -1
    assert lib.rayen_soft_cost_stream_f64(None, None, 0, 1, None, None, None, None, 0, None) == -1


@pytest.mark.parametrize("kernel", ["stream", "auto"])
def test_host_tensors_take_the_mirror_under_every_kernel(kernel):
    c = cost_cases.case("k17_m33")
    y = torch.from_numpy(c.y.copy())
    outs = []
    for sc in (SoftCost(c.cs), SoftCost(c.cs, kernel=kernel)):
        yy = y.clone().requires_grad_(True)
        cost = sc(yy)
        cost.sum().backward()
        outs.append((cost.detach(), yy.grad, *sc.violation(yy)))
    assert all(torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) for a, b in zip(*outs))
    y3 = y.float().unsqueeze(2)
    assert torch.equal(CostComputer(c.cs, fused=True, kernel=kernel).getSumSoftCostAllSamples(y3),
                       CostComputer(c.cs, fused=True).getSumSoftCostAllSamples(y3))


def test_an_unknown_kernel_is_a_value_error():
    c = cost_cases.case("box3")
    with pytest.raises(ValueError):
        SoftCost(c.cs, kernel="bogus")
    with pytest.raises(ValueError):
        CostComputer(c.cs, fused=True, kernel="bogus")
    with pytest.raises(ValueError):
        CostComputer(c.cs, kernel="stream")          # (a route of the fused soft cost only)
    assert SoftCost(c.cs).kernel == "resident" and SoftCost(c.cs, kernel="auto").kernel == "auto"
    np.testing.assert_array_equal(SoftCost(c.cs, kernel="stream").arrays["A1"], SoftCost(c.cs).arrays["A1"])
