"""The structured LMI cases of tests/lmi_structured_cases.py, proven well-posed with the reference alone (no GPU): they
build, their fp64 truth is finite and feasible, the closed forms agree with it, LAPACK's fp32 arithmetic stays far inside
the fp32 bar, the twin cases cannot be passed by a solver that loses the coupling entry, and the rows the gradient check
sets aside stay a handful."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lmi_structured_cases as S                              # noqa: E402
from helpers import rel_err_rows                              # noqa: E402

NAMES = sorted(S.CASES)
SIZES = {          # the sizes each kernel family is swept at
    ("quad", "float32"): {1, 2, 3, 4, 5, 9, 16, 17, 32}, ("quad", "float64"): {1, 2, 3, 4, 5, 9, 16, 17},
    ("lane", "float32"): {2, 5, 16}, ("lane", "float64"): {2, 5, 16},
    ("wave", "float32"): {33, 64, 65}, ("wave", "float64"): {25, 44},
    ("block", "float32"): {33, 65, 66, 129, 282}, ("block", "float64"): {45, 65, 129},
}


def test_the_table_names_cases_at_the_sizes_of_its_family():
    assert len(set(S.TRIPLES)) == len(S.TRIPLES)
    for name, family, dtype_name in S.TRIPLES:
        c = S.case(name)
        assert c.r in SIZES[family, dtype_name], (name, family, dtype_name)
        if c.r == 282:
            assert c.structure in ("twin", "blockdiag")
        if c.structure == "twin":          # the ratio of the precision, or a control
            ratio = S.CASES[name][1]["ratio"]
            assert ratio in ((1e-4 if dtype_name == "float32" else 7e-9), 1e-2, 1e-5)
        if c.structure in ("graded3", "graded6"):
            assert c.structure == ("graded3" if dtype_name == "float32" else "graded6")
    # every structure at a size that is a multiple of 4 and at one that is not, wherever the family has both
    # (the workgroup kernel's sizes hold no multiple of 4: two sizes stand in; W_21 fits one of the quad kernel's sizes)
    for (family, dtype_name), sizes in SIZES.items():
        names = [n for n, f, d in S.TRIPLES if (f, d) == (family, dtype_name)]
        for structure in {S.case(n).structure for n in names}:
            got = {S.case(n).r for n in names if S.case(n).structure == structure}
            if structure == "wilkinson" and family == "quad":
                continue
            assert len(got) >= 2, (family, dtype_name, structure)
            if any(s % 4 == 0 for s in sizes if s >= 4):
                assert any(s % 4 == 0 for s in got) and any(s % 4 for s in got), (family, dtype_name, structure, got)
    assert {n for n, _, _ in S.TRIPLES} | {v[0] for v in S.COST_SETS.values()} == set(S.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_case_builds_and_its_truth_is_feasible(name):
    c = S.case(name)
    assert not np.any(c.raw["y0"]) and np.array_equal(c.raw["F"][-1], np.eye(c.r))
    for Fa in c.raw["F"]:
        assert np.array_equal(Fa, Fa.T)
    cs, ev = S.truth(name)
    assert cs.n == c.k and np.array_equal(cs.NA_E, np.eye(c.k))
    assert np.all(np.isfinite(ev["y"])) and np.all(np.isfinite(ev["kappa"])) and np.all(ev["kappa"] >= 0)
    assert cs.getMaxViolation(ev["y"]) <= 1e-9
    assert not np.any(ev["y"][2])                              # row 2 returns y0 = 0
    if not name.endswith(("_1e4", "_1e8")):                    # rows 0-1 are interior (generators of 1e4 and more undo their 1e-4)
        assert np.all(ev["kappa"][:2] < 1)
        assert np.allclose(ev["y"][:2], c.x[:2], rtol=1e-14, atol=0)
    # the oracle's LMI term IS lambda_max(S): the reference's Cholesky factor is I
    lam = S.spectrum(c.raw, c.x)[:, -1]
    assert np.allclose(np.maximum(lam, 0.0), ev["kappa"], rtol=1e-11, atol=1e-13 * max(1.0, np.abs(lam).max()))


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("diag")])
def test_diagonal_lmi_is_its_polytope(name):
    c = S.case(name)
    _, ev = S.truth(name)
    lin = S.evaluate(S.build(S.polytope_raw(c.raw)), c.x)
    assert rel_err_rows(lin["y"], ev["y"]).max() <= 1e-12


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith(("identity_", "toeplitz"))])
def test_intervals_in_closed_form(name):
    c = S.case(name)
    _, ev = S.truth(name)
    bound = -1.0 if name.startswith("identity") else S.toeplitz_bound(c.r)
    assert rel_err_rows(np.maximum(c.x, bound), ev["y"]).max() <= 1e-12


def test_lapack_fp32_is_far_inside_the_fp32_bar():
    """The reference's own fp32 arithmetic against the fp64 truth, every case: at most 2e-6, so the fp32 bar of the device
    tests, ``max(1e-5, 2 x this)``, is the flat 1e-5 on every case.  The largest value over the table: 1.79e-6
    (scaled_r65_1e8), then 1.73e-6 (zero_line_r65_j64) and 1.67e-6 (blockdiag_150_132): the dense blocks of 64 rows and
    more sit between 1.2e-6 and 2.7e-6 depending on the seed, and the seeds of scaled_r64_1e4, scaled_r66_1e4 and
    zero_line_r66_j0 were moved on for this bound."""
    worst = {name: float(S.lapack32_error(name).max()) for name in NAMES}
    top = max(worst, key=worst.get)
    print(f"LAPACK fp32 against fp64: worst {worst[top]:.3e} ({top})")
    assert worst[top] <= 2e-6, (top, worst[top])


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("twin")])
def test_twin_cases_are_sensitive_to_the_coupling_entry(name):
    """lambda_max with the coupling entries zeroed moves by 2.5 bars or more on a third of the rows or more: a solver that
    discards them cannot pass (the controls at 1e-5 are exempt: there the loss is below the bar by construction)."""
    c = S.case(name)
    ratio = S.CASES[name][1]["ratio"]
    lam = S.spectrum(c.raw, c.x)[:, -1]
    cut = S.spectrum(S.twin_without_delta(c.raw), c.x)[:, -1]
    assert np.count_nonzero(S.twin_without_delta(c.raw)["F"][0]) == 4 and np.count_nonzero(c.raw["F"][0]) == 6
    move = np.abs(lam - cut) / np.maximum(np.abs(lam), 1e-300)
    on_top = move > 0.4 * ratio                                # rows whose top eigenvalue is the twin's: c + delta / 2
    assert np.allclose(move[on_top], 0.5 * ratio, rtol=5e-3)       # (c + delta / 2 to first order in delta / c)
    assert on_top.sum() >= c.B / 3
    if ratio == 1e-5:
        return
    bar = S.BAR["float32" if ratio in (1e-4, 1e-2) else "float64"]
    if ratio == 1e-2:          # a control of both precisions
        bar = S.BAR["float32"]
    assert (move >= 2.5 * bar).sum() >= c.B / 3, (name, np.sort(move)[-5:])
    # ... and in y, the quantity the device tests compare: the rows outside the set move by as much
    cs_cut = S.build(S.twin_without_delta(c.raw))
    moved = rel_err_rows(S.evaluate(cs_cut, c.x)["y"], S.truth(name)[1]["y"])
    assert (moved >= 2.5 * bar).sum() >= c.B / 3, (name, np.sort(moved)[-5:])


@pytest.mark.parametrize("name,dtype_name", sorted({(n, d) for n, _, d in S.BACKWARD_SEPARATED}))
def test_kink_cap_of_the_gradient_cases(name, dtype_name):
    """The rows tests/test_gpu_lmi_wave.py::_check_backward's rule sets aside, from the fp64 reference alone."""
    c = S.case(name)
    _, ev = S.truth(name)
    kink = S.kinks(ev["terms"], ev["kappa"], dtype_name)
    assert kink.sum() <= max(3, 0.05 * c.B), (name, int(kink.sum()))
