"""The cases of the soft-cost sweep (tests/cost_sweep_cases.py) on the host, before any of them reaches a device: the torch
mirror of ``rayen_amd.soft_cost`` in fp64 and fp32 sits inside the bars the kernels are held to, the index-coverage batches
cover every stacked index, the exact cases are exact in fp32, and the image-size formulas give the limits the kernels state."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cost_cases                                             # noqa: E402
import cost_reference                                         # noqa: E402
import cost_sweep_cases as sweep                              # noqa: E402
from helpers import cost_check                                # noqa: E402
from rayen_amd.soft_cost import _NAMES, Constants, mirror      # noqa: E402

CASES = sweep.all_cases()


def _mirror(c, dtype_name):
    dtype = getattr(torch, dtype_name)
    tensors = {name: torch.from_numpy(np.asarray(c.arrays[name], dtype=np.float64)) for name in _NAMES}
    consts = Constants(tensors, c.arrays["soc_rows"], dtype, "cpu")
    y = torch.from_numpy(c.y.copy()).to(dtype).requires_grad_(True)
    cost, worst, which = mirror(consts, y)
    cost.sum().backward()
    return cost.detach(), worst, which, y.grad


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("name", list(CASES))
def test_mirror_sits_inside_the_bars(name, dtype_name):
    c = CASES[name]()
    cost_check(c, dtype_name, *_mirror(c, dtype_name), f"{name} {dtype_name} mirror")
    bad = np.isnan(c.ref["cost"])
    assert bad.sum() == (1 if c.kind == "nan" else 0)
    if c.kind == "nan":
        clean = sweep.width_case(sweep.NAN_K).ref
        assert np.array_equal(c.ref["cost"][~bad], clean["cost"][~bad]) and np.array_equal(c.ref["grad"][~bad], clean["grad"][~bad])


def test_the_widths_reach_every_fp64_instantiation_on_both_sides_of_each_cut_over():
    Ks = {k: sweep.lane64_K(k) for k in sweep.WIDTHS}
    assert set(Ks.values()) == {8, 16, 32, 64}
    for below, above in ((8, 9), (16, 17), (32, 33)):
        assert Ks[below] == below and Ks[above] == 2 * below
    # 16-byte pieces: vectorisable widths below 64 (some pieces load, the rest zero-fill), and widths in the upper half
    assert {k for k in sweep.WIDTHS if k % 4 == 0 and k < 64} >= {4, 8, 36, 60}
    assert {k for k in sweep.WIDTHS if k > 32} == {33, 36, 60, 63, 64}
    for k in sweep.WIDTHS:
        a = sweep.width_case(k).arrays
        assert (a["b1"].size, a["r"].size, list(a["soc_rows"]), a["b2"].size) == (5, 1, [3], 1)
        assert sweep.served_by_formula(a, "float32") and sweep.served_by_formula(a, "float64")


def test_tile_sets_hold_the_row_counts_of_the_sweep():
    sets = sweep.TILE_SETS
    assert {s[0] for s in sets.values()} >= {0, 1, 31, 32, 33, 65}
    assert {s[3] for s in sets.values()} >= {0, 1, 32, 33, 65}
    assert {r for s in sets.values() for r in s[2]} >= {1, 31, 32, 33, 63, 64, 65}
    assert {s[1] for s in sets.values()} >= {0, 1, 3}
    assert sets["mixed"] == (33, 3, (33, 5, 64), 33)
    for name, (m1, nq, rows, m2) in sets.items():
        a = sweep.tile_set(name)
        assert (a["b1"].size, a["r"].size, tuple(a["soc_rows"]), a["b2"].size, a["k"]) == (m1, nq, rows, m2, sweep.TILE_K)
        assert sweep.served_by_formula(a, "float64")
        assert sweep.served_by_formula(a, "float32") == (name not in sweep.TILE_REFUSED32)


@pytest.mark.parametrize("name", sweep.COVERAGE)
def test_every_stacked_index_is_the_decided_worst_of_a_row(name):
    c = sweep.coverage_case(name)
    n = sweep.n_values(c.arrays)
    assert np.array_equal(c.y, c.y.astype(np.float32).astype(np.float64))          # both precisions read the same rows
    dvals = cost_reference.bounds(c.ref, 2.0 ** -24)[0]
    decided = cost_reference.which_is_decided(c.ref, dvals)
    assert decided.all()
    never = sweep.COVERAGE_UNREACHABLE[name]
    assert sorted(c.ref["which"].tolist()) == [j for j in range(n) if j not in never]
    # what is left out CANNOT be reported: a linear row's margin over the other values is concave in y (a linear function
    # minus a maximum of convex ones), its maximum is negative, so the row is below another value at every y
    for j in never:
        assert j < c.arrays["b1"].size and not c.arrays["b2"].size
        for start in (c.y[0], c.y[-1], np.zeros(c.arrays["k"])):
            assert sweep.best_margin(c.arrays, j, start)[1] < -0.01


@pytest.mark.parametrize("name", list(sweep.EXACT))
def test_exact_cases_are_exact_in_fp32(name):
    c = sweep.EXACT[name]()
    assert sweep.exact_premises(c)
    ref, ref32 = c.ref, cost_reference.reference(c.arrays, c.y.astype(np.float32).astype(np.float64))
    assert all(np.array_equal(ref[key], ref32[key]) for key in ("cost", "worst", "which", "grad"))
    vals, which = ref["vals"], ref["which"]
    if name == "ties":
        for sample, lowest, tied in sweep.TIES:
            assert which[sample] == lowest == min(tied)
            assert np.all(vals[sample, list(tied)] == ref["worst"][sample])
            others = np.delete(vals[sample], list(tied))
            assert np.all(others < ref["worst"][sample])
        assert set(which.tolist()) >= {1, 2, 3, 41}
    if name == "zero":
        rows = list(sweep.ZERO_ROWS)
        assert np.all(ref["worst"][rows] == 0) and np.all(ref["cost"][rows] == 0) and not np.any(ref["grad"][rows])
        assert set(which[rows].tolist()) == {0, 1, 3, 4, 5}               # linear rows, the quadratic and the cone sit at 0
        others = [b for b in range(len(which)) if b not in rows]
        assert np.all(ref["cost"][others] > 0)
    if name == "apex":
        a, rows = c.arrays, list(sweep.APEX_ROWS)
        assert a["soc_rows"][0] < a["k"] and not np.any(a["s"])
        u = c.y @ a["M"].T + a["s"]
        on_apex = ~np.any(u, axis=1)
        assert on_apex[rows].all() and on_apex.sum() == len(rows) + 1
        g = -(c.y @ a["c"][0]) - a["d"][0]
        assert np.all(g[rows] > 0) and np.all(g[on_apex & ~np.isin(np.arange(len(g)), rows)] < 0)
        assert np.array_equal(ref["grad"][rows], -2.0 * g[rows, None] * a["c"][0][None, :])
        assert np.array_equal(ref["cost"][rows], g[rows] ** 2) and np.array_equal(ref["worst"][rows], g[rows])
    if name == "lone_lane":
        assert np.flatnonzero(ref["cost"] > 0).tolist() == [17] and np.all(ref["worst"][np.arange(65) != 17] < 0)
        assert np.flatnonzero(np.any(ref["grad"] != 0, axis=1)).tolist() == [17]
        assert np.all(ref["act"][17, :33].reshape(-1) >= 0) and (ref["act"][17, :32] > 0).any() and ref["act"][17, 33] > 0


def test_image_formulas_give_the_limits():
    assert sweep.image_bytes32(608, 0, (), 0) == 19 * (2048 + 32 + 8) * 4 == 158688 <= sweep.LDS_BUDGET
    assert sweep.image_bytes32(609, 0, (), 0) > sweep.LDS_BUDGET
    assert sweep.limit_rows("float32") == 608
    m64 = sweep.limit_rows("float64")
    # fp64 at k = 8: 8 m (rows) + m (constants) + 1 (fconst) + 4 (one descriptor) words of 8 bytes
    assert m64 == (sweep.LDS_BUDGET // 8 - 5) // 9 == 2275
    assert sweep.image_bytes64(m64, 0, (), 0, 8) <= sweep.LDS_BUDGET < sweep.image_bytes64(m64 + 1, 0, (), 0, 8)
    for d in ("float32", "float64"):
        m = sweep.limit_rows(d)
        assert sweep.served_by_formula(sweep.limit_case(m).arrays, d)
        assert not sweep.served_by_formula(sweep.limit_case(m + 1).arrays, d)
        assert not sweep.served_by_formula(sweep.k65_case().arrays, d)
    # the seeded cases of tests/cost_cases.py: all served, but config 3 in fp64 (520 stacked rows of 64 columns)
    for name in ("box3", "lin5_eq2", "quad_soc7", "k17_m33", "c3"):
        a = cost_cases.case(name).arrays
        assert sweep.served_by_formula(a, "float32")
        assert sweep.served_by_formula(a, "float64") == (name != "c3")
    a = cost_cases.case("c3").arrays
    assert 260 * 1024 < sweep.image_bytes64(a["b1"].size, a["r"].size, [int(r) for r in a["soc_rows"]], a["b2"].size, a["k"]) < 270 * 1024


def test_multi_round_batches_take_a_second_round():
    """The grid of rayen_launch_geometry.h: groups dealt over the resident waves in equal rounds."""
    for cus in (sweep.NOMINAL_CUS, 64, 304):
        slots32, B32 = 4 * cus, sweep.rounds_batch(cus, "float32")
        assert -(-(-(-B32 // 32)) // slots32) == 2
        B64 = sweep.rounds_batch(cus, "float64")
        assert -(-(-(-B64 // 256)) // cus) == 2


def test_infinite_input_gives_an_infinite_cost_in_the_reference():
    y, a = sweep.inf_case()
    with np.errstate(all="ignore"):
        ref = cost_reference.reference(a, y)
    rows = list(sweep.INF_ROWS)
    assert np.all(ref["cost"][rows] == np.inf) and np.all(ref["worst"][rows] == np.inf) and np.all(ref["which"][rows] == 0)
    assert np.all(np.isfinite(np.delete(ref["cost"], rows)))
