"""``rayen_amd.soft_cost.SoftCost`` on the host: its torch-ops mirror against the fp64 reference written out one constraint
at a time (tests/cost_reference.py), autograd, the LMI detour, ``CostComputer(fused=True)`` and the module plumbing."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cost_cases                                             # noqa: E402
from rayen_amd import workloads                               # noqa: E402
from rayen_amd.cost_computer import CostComputer              # noqa: E402
from rayen_amd.soft_cost import SoftCost, mirror_values                    # noqa: E402


@pytest.mark.parametrize("name", cost_cases.NAMES)
def test_seeded_cases_are_well_posed(name):
    """What the GPU bars assume: no cone of a seeded case is evaluated near its apex (||My + s|| below 1e-3 of its scale), and
    the inside / outside batches are what they say."""
    c = cost_cases.case(name)
    assert c.ref["soc_min_ratio"] >= 1e-3
    if c.kind == "inside":
        assert np.all(c.ref["worst"] < 0) and np.all(c.ref["cost"] == 0) and np.all(c.ref["grad"] == 0)
    if c.kind == "outside":
        assert np.all(c.ref["worst"] > 0)
    if c.kind == "mixed" and c.y.shape[0] > 1:
        assert np.any(c.ref["worst"] > 0)


@pytest.mark.parametrize("name", cost_cases.NAMES)
def test_mirror_against_the_reference_fp64(name):
    c = cost_cases.case(name)
    ref = c.ref
    sc = SoftCost(c.cs)
    y = torch.from_numpy(c.y.copy()).requires_grad_(True)
    cost = sc(y.unsqueeze(2))
    cost.sum().backward()
    worst, which = sc.violation(y)
    bad = np.isnan(ref["cost"])
    assert np.array_equal(np.isnan(cost.detach().numpy()), bad) and np.array_equal(np.isnan(worst.numpy()), bad)
    assert bad.sum() == (1 if c.kind == "nan" else 0)
    ok = ~bad
    g, e = mirror_values(sc.constants(torch.float64, "cpu"), y.detach())
    vals = torch.cat((g, e.abs()), dim=1).numpy()
    assert np.all(np.abs(vals - ref["vals"])[ok] <= 1e-12 * ref["S"][ok])          # every value, relative to ITS scale
    scale = np.max(ref["S"], axis=1)                        # the largest condition scale of the row's values
    assert np.all(np.abs(worst.numpy() - ref["worst"])[ok] <= 1e-12 * scale[ok])
    # cost and gradient: relative to the scale of their own terms (products of two values / a value and a direction)
    assert np.all(np.abs(cost.detach().numpy() - ref["cost"])[ok] <= 1e-12 * np.sum(ref["S"] ** 2, axis=1)[ok])
    gscale = sum(2.0 * ref["S"][:, j:j + 1] * np.abs(ref["dirs"][j]) for j in range(ref["S"].shape[1]))
    assert np.all(np.abs(y.grad.numpy() - ref["grad"])[ok] <= 1e-12 * (gscale[ok] + 1e-300))
    assert np.all(np.isnan(y.grad.numpy()[bad]))
    dvals = cost_cases.cost_reference.bounds(ref, 2.0 ** -53)[0]
    decided = cost_cases.cost_reference.which_is_decided(ref, dvals)
    assert np.array_equal(which.numpy()[decided], ref["which"][decided])
    assert np.all(which.numpy()[bad] == -1)
    if c.kind == "inside":
        assert np.all(cost.detach().numpy() == 0) and np.all(y.grad.numpy() == 0) and np.all(worst.numpy() < 0)


@pytest.mark.parametrize("name", ["box3", "lin5_eq2"])
def test_mirror_gradcheck(name):
    c = cost_cases.case(name)
    sc = SoftCost(c.cs)
    y = torch.from_numpy(c.y[:4].copy()).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: sc(t), (y,), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_fused_cost_computer_equals_the_plain_one():
    torch.set_default_dtype(torch.float64)
    try:
        for raw in (workloads.make_raw("c2", seed=1), workloads.corridor_like(k=12, n_eq=3, m=20, n_quad=3, rank=2, seed=2),
                    workloads.random_lin_quad_soc(k=7, m=5, n_quad=1, n_soc=2, seed=3)):
            cs = workloads.build_constraints(raw)
            y = torch.tensor(np.random.default_rng(0).uniform(-2, 2, size=(40, cs.k))).unsqueeze(2)
            ya, yb = y.clone().requires_grad_(True), y.clone().requires_grad_(True)
            plain, fused = CostComputer(cs), CostComputer(cs, fused=True)
            a, b = plain.getSumSoftCostAllSamples(ya), fused.getSumSoftCostAllSamples(yb)
            assert abs(a.item() - b.item()) <= 1e-12 * abs(a.item())
            a.backward()
            b.backward()
            assert torch.allclose(ya.grad, yb.grad, rtol=1e-10, atol=1e-10 * float(ya.grad.abs().max()))
            assert torch.equal(plain.getInequalityValues(y), fused.getInequalityValues(y))
            assert not plain.fused and "soft_cost.A1" not in plain.state_dict()
    finally:
        torch.set_default_dtype(torch.float32)


def test_lmi_set_runs_the_mirror():
    cs = workloads.build_constraints(workloads.random_lmi(4, 5, seed=1))
    sc = SoftCost(cs)
    rng = np.random.default_rng(3)
    y = np.concatenate((0.05 * rng.standard_normal((5, 4)), 3.0 * rng.standard_normal((6, 4))), axis=0)
    yt = torch.from_numpy(y).requires_grad_(True)
    worst, which = sc.violation(yt)
    res = cs.getResiduals(y)
    assert np.allclose(worst.numpy(), cs.getViolationRows(y), rtol=0, atol=1e-12)
    assert np.all(which.numpy() == 0)                         # the LMI is the set's only constraint
    cost = sc(yt)
    want = np.maximum(res["lmi"], 0.0) ** 2                   # relu(-lambda_min)^2
    assert np.allclose(cost.detach().numpy(), want, rtol=1e-12, atol=1e-14)
    assert np.any(want > 0) and np.any(want == 0)
    cost.sum().backward()
    g = yt.grad.numpy()
    assert np.all(np.isfinite(g))
    assert np.all(np.abs(g[want > 0]).max(axis=1) > 0) and np.all(g[want == 0] == 0)
    with pytest.raises(NotImplementedError):                  # unchanged: the stacked values of CostComputer refuse a LMI
        CostComputer(cs, fused=True).getInequalityValues(yt.detach().unsqueeze(2))


def test_packs_are_rebuilt_never_pickled():
    c = cost_cases.case("quad_soc7")
    sc = SoftCost(c.cs)
    y = torch.from_numpy(c.y.copy())
    want = sc(y)
    assert sc._constants
    sc._cost_packs[0] = (object(), 1)                         # stands for a device pack
    clone = pickle.loads(pickle.dumps(sc))
    assert clone._cost_packs == {} and clone._constants == {} and clone._unsupported == set()
    assert torch.equal(clone(y), want)
    sc.double()
    assert sc._cost_packs == {} and sc._constants == {}
    sc.float()
    assert sc.A1.dtype == torch.float32 and sc(y.float()).dtype == torch.float32
    half = sc(y.to(torch.bfloat16))                           # 16-bit inputs: computed in fp32
    assert half.dtype == torch.bfloat16
