"""The fp64 reference and the bars of tests/cost_lmi_cases.py (soft cost of sets with an LMI), checked on the host before the
GPU tests rely on them: the reference against the torch mirror and against ``ConvexConstraints.getResiduals``, the gap
condition of every case, and the bars themselves -- they reject five deliberately wrong answers built from the reference's
own output and accept the mirror run in fp32."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cost_lmi_cases as L                                    # noqa: E402
from rayen_amd.soft_cost import SoftCost                      # noqa: E402

CASES = [(n, B) for n in L.SERVED for B in L.BATCHES]


def test_limits_are_the_documented_ones():
    assert (L.R_MAX32, L.R_MAX64) == (192, 135)               # "about 190 and 135" (include/rayen_hip.h)
    assert L.served("k5_rmax32", "float32") and not L.served("k5_over32", "float32")
    assert L.served("k5_rmax64", "float64") and not L.served("k5_over64", "float64") and L.served("k5_over64", "float32")
    assert not L.served("k5_rmax32", "float64")


@pytest.mark.parametrize("name,B", CASES)
def test_reference_against_the_mirror_and_the_residuals(name, B):
    c = L.case(name, B)
    ref, ok = c.ref, c.finite
    sc = SoftCost(c.cs)
    y = torch.from_numpy(c.y.copy()).requires_grad_(True)
    cost = sc(y)
    cost.sum().backward()
    worst, which = sc.violation(y)
    cost, worst, which, grad = cost.detach().numpy(), worst.numpy(), which.numpy(), y.grad.numpy()
    assert np.array_equal(np.isnan(cost), ~ok) and np.array_equal(np.isnan(worst), ~ok) and np.all(which[~ok] == -1)
    size = np.where(ok, np.maximum(np.max(np.abs(np.where(ok[:, None], ref["vals"], 0.0)), axis=1), 1.0), 1.0)
    assert np.all(np.abs(worst - ref["worst"])[ok] <= 1e-10 * size[ok])
    assert np.all(np.abs(cost - ref["cost"])[ok] <= 1e-10 * np.maximum(ref["cost"], 1.0)[ok])
    decided = ok & (np.abs(worst - ref["worst"]) < 1e-300) if ref["vals"].shape[1] == 1 else ok
    top2 = np.sort(np.where(ok[:, None], ref["vals"], 0.0), axis=1)[:, -2:] if ref["vals"].shape[1] > 1 else None
    if top2 is not None:
        decided = ok & (top2[:, 1] - top2[:, 0] > 1e-9 * size)
    assert np.array_equal(which[decided], ref["which"][decided])
    kept = c.kept
    gsize = np.maximum(np.max(np.abs(np.where(ok[:, None], ref["grad"], 0.0)), axis=1), 1e-300)
    assert np.all(np.abs(grad - ref["grad"])[kept] <= 1e-10 * np.maximum(gsize, 1.0)[kept, None])
    # the residuals the set itself reports
    yf = c.y[ok]
    assert np.all(np.abs(c.cs.getResiduals(yf)["lmi"] - ref["lmi"]["g"][ok]) <= 1e-12 * ref["lmi"]["scale"][ok])
    assert np.all(np.abs(c.cs.getViolationRows(yf) - ref["worst"][ok]) <= 1e-12 * size[ok])


@pytest.mark.parametrize("name,B", CASES)
def test_gap_condition_and_row_kinds(name, B):
    c = L.case(name, B)
    lmi = c.ref["lmi"]
    assert (c.kept | c.degenerate)[c.finite].sum() >= 0.75 * c.finite.sum()
    assert np.all(lmi["gap"][c.kept] >= 1e-2) and not np.any(c.kept & c.degenerate)
    kinds = np.array(c.kinds)
    assert (~c.finite).sum() == (kinds == "nan").sum()
    for b in np.flatnonzero(kinds == "degenerate"):           # F(y) = ALPHA I: every eigenvalue the same, outside the set
        H = c.arrays["F"][-1] + np.tensordot(c.y[b], c.arrays["F"][:-1], axes=1)
        assert np.allclose(H, L.ALPHA * np.eye(c.r), atol=1e-14) and abs(lmi["g"][b] + L.ALPHA) <= 1e-14
    if B == 67:
        assert np.all(lmi["g"][kinds == "interior"] < -0.1) and np.all(c.ref["lmi_cost"][kinds == "interior"] == 0)
        assert np.all(c.ref["lmi_grad"][kinds == "interior"] == 0)
        assert (lmi["g"][kinds == "outside"] > 0.1).sum() >= 12
        near = np.abs(lmi["g"] / lmi["scale"])[kinds == "near"]
        assert ((near > 2e-6) & (near < 5e-5)).sum() >= 6 and ((near > 2e-10) & (near < 5e-9)).sum() >= 6


def _answers(c, dtype_name):
    ref, _ = c.reference_for(dtype_name)
    return ref, dict(cost=ref["cost"].copy(), worst=ref["worst"].copy(), which=ref["which"].copy(), grad=ref["grad"].copy())


def _relu(g):
    return np.where(g < 0, 0.0, g)


@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
def test_bars_accept_the_reference_and_reject_wrong_answers(dtype_name):
    alone, mixed = L.case("k10_r20", 67), L.case("lin5_eq2_lmi8", 67)
    for c in (alone, mixed):
        ref, a = _answers(c, dtype_name)
        L.check(c, dtype_name, a["cost"], a["worst"], a["which"], a["grad"], "reference")

    def rejected(c, what, **wrong):
        _, a = _answers(c, dtype_name)
        a.update(wrong)
        with pytest.raises(AssertionError):
            L.check(c, dtype_name, a["cost"], a["worst"], a["which"], a["grad"], what)

    ref, _ = _answers(alone, dtype_name)
    g, w = ref["lmi"]["g"], ref["lmi"]["w"]
    # the sign of g
    rejected(alone, "sign", cost=_relu(-g) ** 2, worst=-g, grad=-2.0 * _relu(-g)[:, None] * w)
    # lambda_max in place of lambda_min
    gmax = -ref["lmi"]["lam_max"]
    rejected(alone, "lambda_max", cost=_relu(gmax) ** 2, worst=gmax, grad=2.0 * _relu(gmax)[:, None] * w)
    # a gradient missing the factor 2 (values right)
    rejected(alone, "factor 2", grad=0.5 * ref["grad"])
    # mixed set: which without the +1 shift of the equalities; an accumulate that overwrites cost
    ref, _ = _answers(mixed, dtype_name)
    which = ref["which"].copy()
    assert np.any(which > ref["lmi_id"]) and np.any(which == ref["lmi_id"]) and np.any((which >= 0) & (which < ref["lmi_id"]))
    rejected(mixed, "shift", which=np.where(which > ref["lmi_id"], which - 1, which).astype(np.int32))
    rejected(mixed, "overwrite", cost=np.where(np.isnan(ref["cost"]), np.nan, ref["lmi_cost"]))
    # each of the above is a defect of ONE output: with it put right the answers pass again
    _, a = _answers(mixed, dtype_name)
    L.check(mixed, dtype_name, a["cost"], a["worst"], a["which"], a["grad"], "reference again")


@pytest.mark.parametrize("name", L.SERVED)
def test_bars_accept_the_mirror_in_fp32(name):
    c = L.case(name, 67)
    sc = SoftCost(c.cs).float()
    y = torch.from_numpy(c.y.astype(np.float32)).requires_grad_(True)
    cost = sc(y)
    cost.sum().backward()
    worst, which = sc.violation(y)
    L.check(c, "float32", cost.detach().numpy(), worst.numpy(), which.numpy(), y.grad.numpy(), f"{name} mirror fp32")
