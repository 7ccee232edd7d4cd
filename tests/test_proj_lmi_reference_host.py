"""Host checks of the Euclidean projection onto sets with an LMI (``lmi=True``): the program and its svec block, the
mirror of rayen_amd/projection.py against the fp64 reference of tests/proj_lmi_reference.py, the Jacobian reference against
finite differences, and ``compare`` against deliberately defective mirrors.  No GPU."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import proj_lmi_reference as L                               # noqa: E402
from rayen_amd import projection                             # noqa: E402

NAMES = [c.name for c in L.CASES]
# Central differences of project_rows with step h = 1e-5: the solve stops at 1e-11, so each difference carries up to
# 2e-11 / 2e-5 = 1e-6 of solver noise, and O(h^2) = 1e-10 of truncation.  Measured on these rows: 2e-11 .. 5e-9.
FD_STEP, FD_BAR = 1e-5, 1e-6
FD_CASES = ["r1_k1", "r2_psd_cone_isometric", "r3_k4", "r6_identity_offset", "r8_k6", "k8_eq3_lin5_lmi5", "quad_soc_lmi7"]


def test_default_still_raises_and_the_keyword_builds():
    cs = L.make_cs("r3_k4")
    with pytest.raises(NotImplementedError, match="lmi=True"):
        projection.build_program(cs)
    with pytest.raises(NotImplementedError, match="lmi=True"):
        projection.ProjectionModule(cs, create_map=False)
    with pytest.raises(NotImplementedError, match="lmi=True"):
        cs.projectBatch(np.zeros((1, cs.k)))
    prog = projection.build_program(cs, lmi=True)
    assert (prog.psd_dim, prog.psd_row0, prog.m) == (3, 0, 6)
    arrays = prog.arrays()
    assert arrays["psd_dim"] == 3 and arrays["psd_row0"] == 0
    assert projection.ProjectionModule(cs, create_map=False, lmi=True).program.psd_dim == 3


@pytest.mark.parametrize("name", NAMES + [L.REFUSED.name])
def test_shapes_and_served_restated(name):
    assert L.shape_of(name) == L.SHAPE[name]
    n, m, n_soc, r = L.SHAPE[name]
    prog = L.module_for(name).program
    assert prog.psd_row0 == m - r * (r + 1) // 2 == prog.m_lin + sum(prog.soc_rows)
    for dtype_name, elem in (("float32", 4), ("float64", 8)):
        assert L.case_served(name, dtype_name) == (name != L.REFUSED.name)
        assert L.lds_bytes(n, m, r, elem) == (L.pr.lds_bytes(n, m, elem) // elem + L.WAVES * L.psd_scratch(r)) * elem


def test_served_limits():
    assert L.SHAPE["quad_soc_lmi7"][1] - 28 == 18                          # psd_row0 is no multiple of 64
    assert L.served(4, 528, 0, 32, 4) and L.served(4, 528, 0, 32, 8)       # the largest block: 528 rows, 9 per lane
    assert L.served(4, 576, 0, 32, 4) and not L.served(4, 577, 0, 32, 4)   # 528 rows plus the rest stay within 576
    assert not L.served(2, 561, 0, 33, 4)
    assert L.served(64, 522, 6, 0, 4) == L.pr.served(64, 522, 6, 4)        # no block: the rule of proj_reference
    assert L.lds_bytes(4, 528, 32, 8) == 146752                            # the LDS budget at r = 32 in fp64
    assert not L.served(64, 576, 0, 32, 4)                                 # image + scratch over 160 KiB


@pytest.mark.parametrize("name", ["r3_k4", "quad_soc_lmi7"])
def test_svec_is_isometric_and_the_block_is_one_scale_of_F(name):
    cs, module = L.make_cs(name), L.module_for(name)
    c = module.constants(torch.float64, torch.device("cpu"))
    q = torch.from_numpy(L.make_inputs(name)[0][:9])
    block = (q @ c.G.T + c.h)[:, c.psd_row0:]
    M = projection.smat(c, block)
    assert torch.allclose(block.norm(dim=1), M.flatten(1).norm(dim=1), rtol=1e-14, atol=0)
    assert torch.allclose(projection.svec(c, M), block, rtol=1e-15, atol=0)      # (x / sqrt2 * sqrt2: an ulp)
    for b in range(9):
        F = L.lmi_matrix(cs, q[b].numpy())[0]
        ratio = M[b].numpy() / F
        assert np.allclose(ratio, ratio[0, 0], rtol=1e-9, atol=0)            # ONE scale for the whole block


def _psd_known_answer(q):
    lam, V = np.linalg.eigh(np.array([[q[0], q[1] / np.sqrt(2)], [q[1] / np.sqrt(2), q[2]]]))
    P = (V * np.maximum(lam, 0.0)) @ V.T
    return np.array([P[0, 0], np.sqrt(2) * P[0, 1], P[1, 1]])


def test_known_answer_of_the_isometric_cone():
    """``y`` is svec of ``F(y)``: the projection is ``svec(Pi_psd(smat(q)))`` in closed form, no reference involved.  The
    mirror stops at residuals of 1e-9 (1 + |.|); 1e-7 leaves a factor 100 for the conditioning of the fixed point."""
    name = "r2_psd_cone_isometric"
    q, _ = L.make_inputs(name)
    known = np.stack([_psd_known_answer(row) for row in q])
    assert np.any(np.abs(known - q).max(axis=1) > 0.1) and np.any(np.all(known == q, axis=1))
    run = L.mirror_run(name, "float64")
    assert np.max(np.abs(run.z - known)) <= 1e-7
    assert np.max(np.abs(L.reference(name).z - known)) <= 1e-8               # (and the reference solver agrees)
    run32 = L.mirror_run(name, "float32")
    assert np.max(np.abs(run32.z - known)) <= 1e-4


@pytest.mark.parametrize("name", NAMES)
def test_seeded_rows_are_no_coin_toss_and_within_the_kink_cap(name):
    cs, ref = L.make_cs(name), L.reference(name)
    margins = np.array([L.decision_margin(cs, row) for row in ref.q])
    assert margins.min() >= L.DECISION_MARGIN
    for B in L.batches_of(name):
        assert np.count_nonzero(ref.kink[:B]) <= L.kink_cap(B)
    assert ref.interior.any() and not ref.interior.all()
    if name == "r8_k6":
        assert np.count_nonzero(ref.nullity >= 2) > 10                       # nullity above 1 is not an edge case


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("name", NAMES)
def test_mirror_passes_compare(name, dtype_name):
    run = L.mirror_run(name, dtype_name)
    assert L.compare(name, dtype_name, run.z, run.grad_q, run.iters) == []
    assert run.iters.max() < L.MAX_ITERS
    if dtype_name == "float64":
        fwd, bwd, _ = L.bars(name, dtype_name)
        assert fwd <= L.FP64_CAP and bwd <= L.FP64_CAP


@pytest.mark.parametrize("name", FD_CASES)
def test_jacobian_reference_against_finite_differences(name):
    cs, ref = L.make_cs(name), L.reference(name)
    outside = np.flatnonzero(~ref.interior & ~ref.kink)
    rows = list(outside[:2]) + list(outside[ref.nullity[outside] == ref.nullity[outside].max()][:1])
    for b in rows:
        J = L.jacobian_row(cs, ref.q[b], ref.z[b])[0]
        Jfd = np.empty_like(J)
        for j in range(cs.n):
            e = np.zeros(cs.n)
            e[j] = FD_STEP
            zz = L.project_rows(cs, np.stack([ref.q[b] + e, ref.q[b] - e]))
            Jfd[:, j] = (zz[0] - zz[1]) / (2 * FD_STEP)
        print(f"{name} row {b} nullity {ref.nullity[b]}: |J - Jfd| {np.abs(J - Jfd).max():.2e}")
        assert np.abs(J - Jfd).max() <= FD_BAR
        assert np.allclose(J, J.T, atol=1e-9)


def test_a_nan_row_stays_nan_and_alone():
    name = "r3_k4"
    c = L.module_for(name).constants(torch.float64, torch.device("cpu"))
    q = torch.from_numpy(L.make_inputs(name)[0][:9].copy())
    bad = q.clone()
    bad[4, 1] = float("nan")
    z0, it0, v0 = projection.mirror_forward(c, q, 50, 1e-9)
    z1, it1, v1 = projection.mirror_forward(c, bad, 50, 1e-9)
    keep = torch.arange(9) != 4
    assert torch.all(torch.isnan(z1[4])) and int(it1[4]) == 50
    assert torch.equal(z1[keep], z0[keep]) and torch.equal(it1[keep], it0[keep])
    g = torch.ones_like(q)
    g0 = projection.mirror_backward(c, g, v0, it0, 50, 1e-9)
    g1 = projection.mirror_backward(c, g, v1, it1, 50, 1e-9)
    assert torch.all(torch.isnan(g1[4])) and torch.equal(g1[keep], g0[keep])


def test_project_batch_equals_a_loop_of_project():
    name = "k8_eq3_lin5_lmi5"
    cs = L.make_cs(name)
    rng = np.random.default_rng(3)
    Y = cs.y0.reshape(1, -1) + rng.standard_normal((5, cs.k))               # (off the equality subspace too)
    out, dist = cs.projectBatch(Y, lmi=True)
    for b in range(5):
        y, d = cs.project(Y[b])
        assert np.max(np.abs(out[b] - y[:, 0])) <= 1e-6 and abs(dist[b] - d) <= 1e-6


def test_pickle_round_trip():
    name = "r3_k4"
    module = L.module_for(name)
    clone = pickle.loads(pickle.dumps(module))
    assert (clone.program.psd_dim, clone.program.psd_row0) == (module.program.psd_dim, module.program.psd_row0)
    q = torch.from_numpy(L.make_inputs(name)[0][:9])
    z0, it0 = module.project(q)
    z1, it1 = clone.project(q)
    assert torch.equal(z0, z1) and torch.equal(it0, it1)


# ------------------------------------------------------------------------------------------------------------------
# compare rejects defective mirrors
# ------------------------------------------------------------------------------------------------------------------

def _no_sqrt2(monkeypatch):
    real = projection.svec_index
    monkeypatch.setattr(projection, "svec_index", lambda r: real(r)[:2] + (np.ones(r * (r + 1) // 2),))


def _clip_abs(monkeypatch):
    def project(c, v):
        lam, V, _ = projection.psd_eig(c, v)
        rebuilt = projection.svec(c, (V * lam.abs()[:, None, :]) @ V.transpose(1, 2))
        return torch.where((lam >= 0).all(dim=1)[:, None], v[:, c.psd_row0:], rebuilt)
    monkeypatch.setattr(projection, "_psd_project", project)


def _mixed_weight(value):
    def patch(monkeypatch):
        def weights(lam):
            pi, pj = lam[:, :, None] > 0, lam[:, None, :] > 0
            return torch.where(pi & pj, 1.0, torch.where(pi ^ pj, value, 0.0)).to(lam.dtype)
        monkeypatch.setattr(projection, "_psd_weights", weights)
    return patch


def _per_row_scale(monkeypatch):
    def equilibrate(G, h, m_lin, soc_rows, psd_dim=0):
        Gh = np.concatenate((G, h[:, None]), axis=1)
        rn = np.linalg.norm(Gh, axis=1)
        scale = 1.0 / np.where(rn > 0, rn, 1.0)
        return G * scale[:, None], h * scale
    monkeypatch.setattr(projection, "_equilibrate", equilibrate)


def _always_rebuilt(monkeypatch):
    def project(c, v):
        lam, V, _ = projection.psd_eig(c, v)
        return projection.svec(c, (V * torch.clamp_min(lam, 0.0)[:, None, :]) @ V.transpose(1, 2))
    monkeypatch.setattr(projection, "_psd_project", project)


DEFECTS = {"off-diagonals not scaled by sqrt(2)": _no_sqrt2, "|lambda| in place of max(lambda, 0)": _clip_abs,
           "B = 1 on mixed pairs": _mixed_weight(1.0), "B = 0 on mixed pairs": _mixed_weight(0.0),
           "a scale per row of the block": _per_row_scale, "a reconstruction for an interior block": _always_rebuilt}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_compare_rejects_a_defective_mirror(defect, monkeypatch):
    name = "r3_k4"
    DEFECTS[defect](monkeypatch)
    module = projection.ProjectionModule(L.make_cs(name), create_map=False, lmi=True, rho=L.module_for(name).program.rho)
    run = L.run_mirror(module, name, "float64", max_iters=600)
    fails = L.compare(name, "float64", run.z, run.grad_q, run.iters)
    print(defect, "->", fails)
    assert fails != []
