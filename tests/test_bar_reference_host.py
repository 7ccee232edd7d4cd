"""Host checks of tests/bar_reference.py: the closed-form gradient against autograd, and that the sweep's inputs and
tolerance tell a subtly wrong kernel from a right one (each deliberate defect below shows at >= 100 x the tolerance the
GPU sweep applies, on the very inputs that sweep runs)."""
import numpy as np
import pytest
import torch

import bar_reference as br

SEPARATION = 100.0


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _inputs(case, variant):
    B = br.sweep_batches(case)[-1]                        # rows_per_iter + 1: the sweep's largest small batch
    G, yp = br.make_pack(case)
    q, gy = br.make_inputs(case, B, variant)
    return _t(G), _t(yp), _t(q), _t(gy)


@pytest.mark.parametrize("variant", ["plain", "edges"])
@pytest.mark.parametrize("case", br.CASES, ids=lambda c: c.name)
def test_closed_form_gradient_equals_autograd(case, variant):
    G, yp, q, gy = _inputs(case, variant)
    leaf = q.clone().requires_grad_(True)
    br.forward64(G, yp, case.nv, case.nr, leaf).backward(gy)
    got = br.backward64(G, case.nv, case.nr, q, gy)
    err = br.scaled_err(got, leaf.grad, br.backward_scale(G, case.nv, case.nr, q, gy)).max().item()
    assert err <= 1e-13, err
    if variant == "edges":
        m = case.nv + case.nr
        dead = torch.isinf(q[:, :m]) | (q[:, :m] == 0)
        assert dead[:, case.nv:].any() or case.nr == 0
        assert dead[:, :case.nv].any() or case.nv <= 1
        assert torch.all(got[dead] == 0) and torch.isfinite(got).all()
        assert torch.isfinite(q[:, :case.nv]).any(dim=1).all() or case.nv == 0


def test_scales_are_sums_of_absolute_values():
    case = br.CASE["L2_k5_mixed_piece"]
    G, yp, q, gy = _inputs(case, "plain")
    w = br.weights64(case.nv, case.nr, q)
    S = br.forward_scale(G, yp, case.nv, case.nr, q)
    assert torch.allclose(S[3], (G.abs() * w[3]).sum(1) + yp.abs(), rtol=1e-14, atol=0)
    assert torch.all(S >= br.forward64(G, yp, case.nv, case.nr, q).abs() * (1 - 1e-14))
    T = br.backward_scale(G, case.nv, case.nr, q, gy)
    assert torch.all(T * (1 + 1e-14) >= br.backward64(G, case.nv, case.nr, q, gy).abs())
    assert br.scaled_err(S, S, torch.zeros_like(S)).max().item() == 0.0
    assert torch.all(br.scaled_err(S + 1.0, S, torch.zeros_like(S)) > 1e300)     # nothing but tiny guards a zero scale


# ------------------------------------------------------------------------------------------------------------------
# a copy of the reference that takes deliberate defects
# ------------------------------------------------------------------------------------------------------------------

def _mutant(case, G, yp, q, gy, defect):
    """(y, grad_q) of the formula with one defect applied; ``None`` where the defect cannot touch that direction."""
    k, nv, nr = case
    m = nv + nr
    G, yp, q, gy = G.clone(), yp.clone(), q.clone(), gy.clone()
    fwd = bwd = True
    if defect == "drop_last_generator":
        G[:, m - 1] = 0
    elif defect == "swap_in_group":
        a = ((m - 2) // 4) * 4                               # the last aligned group of four with two members
        G[:, [a, a + 1]] = G[:, [a + 1, a]]
    elif defect == "boundary_plus_one":
        nv, nr = nv + 1, nr - 1
    elif defect == "boundary_minus_one":
        nv, nr = nv - 1, nr + 1
    elif defect == "omit_yp":
        yp.zero_()
        bwd = False
    elif defect == "neighbour_grad_y":
        gy = torch.roll(gy, 1, dims=0)
        fwd = False
    y = br.forward64(G, yp, nv, nr, q[:, :m]) if fwd else None
    gq = br.backward64(G, nv, nr, q[:, :m], gy) if bwd else None
    if defect == "zero_last_output":
        y[:, k - 1] = 0
        gy[:, k - 1] = 0
        gq = br.backward64(G, nv, nr, q[:, :m], gy)
    elif defect == "sign_zero_is_one":
        g = gy @ G
        gq[:, nv:] = torch.where(q[:, nv:m] == 0, g[:, nv:], gq[:, nv:])
        y = None
    elif defect == "no_dot_term":
        lam = torch.softmax(q[:, :nv], dim=1)
        gq[:, :nv] = lam * (gy @ G)[:, :nv]
        y = None
    return y, gq


def _applicable(case, defect):
    """Structural only: the defect needs the thing it breaks to exist."""
    nv, nr = case.nv, case.nr
    if defect == "swap_in_group":
        return nv + nr >= 2
    if defect in ("boundary_plus_one", "sign_zero_is_one"):
        return nr >= 1
    if defect in ("boundary_minus_one", "no_dot_term"):
        return nv >= 1
    return True


DEFECTS = ["drop_last_generator", "swap_in_group", "boundary_plus_one", "boundary_minus_one", "omit_yp",
           "zero_last_output", "sign_zero_is_one", "no_dot_term", "neighbour_grad_y"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_the_sweep_separates_a_defect_from_the_reference(defect):
    worst = None
    seen = 0
    for case in br.CASES:
        if not _applicable(case, defect):
            continue
        tol = br.tolerance_factor(case) * br.U[torch.float32]             # the wider of the sweep's two bars
        variant = "edges" if defect == "sign_zero_is_one" else "plain"
        G, yp, q, gy = _inputs(case, variant)
        k, nv, nr = case.k, case.nv, case.nr
        y, gq = _mutant(case[1:], G, yp, q, gy, defect)
        errs = []
        if y is not None:
            errs.append(br.scaled_err(y, br.forward64(G, yp, nv, nr, q), br.forward_scale(G, yp, nv, nr, q)).max().item())
        if gq is not None and not (nv == 1 and nr == 0):     # (one vertex, no ray: the gradient is 0 whatever is read)
            errs.append(br.scaled_err(gq, br.backward64(G, nv, nr, q, gy), br.backward_scale(G, nv, nr, q, gy)).max().item())
        if not errs:
            continue
        for e in errs:                                       # every direction the defect touches must show it
            sep = e / tol
            assert sep >= SEPARATION, (defect, case.name, e, tol, sep)
            worst = sep if worst is None else min(worst, sep)
        seen += 1
    assert seen >= 8
    print(f"{defect}: smallest separation over {seen} cases {worst:.3g} x the sweep's tolerance")


def test_every_kernel_instance_and_lane_width_appears_twice():
    by_K, by_L = {}, {}
    for c in br.CASES:
        by_K.setdefault(br.pad_k(c.k), []).append(c.name)
        by_L.setdefault(br.lanes(c.nv + c.nr), []).append(c.name)
    assert sorted(by_K) == [4, 8, 16, 32, 64] and all(len(v) >= 2 for v in by_K.values())
    assert sorted(by_L) == [1, 2, 4, 8, 16] and all(len(v) >= 2 for v in by_L.values())
    assert {c.k for c in br.CASES} == {1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64}
    ms = [c.nv + c.nr for c in br.CASES]
    assert {m % 4 for m in ms} == {0, 1, 2, 3} and max(ms) >= 1024
    assert {c.nv % 4 for c in br.CASES if c.nr > 0 and c.nv > 0} >= {1, 2, 3}
    assert any(br.pieces(m) % br.lanes(m) for m in ms)
    assert any(c.nv == 0 for c in br.CASES) and any(c.nr == 0 for c in br.CASES)
    assert any(c.nv == 1 for c in br.CASES) and any(c.nr == 1 for c in br.CASES)
