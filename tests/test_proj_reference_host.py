"""Host checks of the Euclidean-projection reference (tests/proj_reference.py), of the host mirror of
rayen_amd/projection.py against it, and of the comparisons tests/test_gpu_proj.py applies to the kernels (no GPU)."""
import pickle
import sys
import os

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import proj_reference as pr                                            # noqa: E402
from rayen_amd import conic, constraints, projection, workloads       # noqa: E402

NAMES = [c.name for c in pr.CASES]
SMALL = NAMES[:5]


# ------------------------------------------------------------------ closed forms of the reference projection
def test_box_is_clip():
    ref = pr.reference("n3_box")
    assert np.max(np.abs(ref.z - np.clip(ref.q, 0.0, 1.0))) <= 1e-9


def test_ball_is_radial_scaling():
    ref = pr.reference("n4_ball_quadratic_only")
    nrm = np.linalg.norm(ref.q, axis=1, keepdims=True)
    assert np.max(np.abs(ref.z - ref.q / np.maximum(nrm, 1.0))) <= 1e-9


def test_half_space_formula():
    ref = pr.reference("n1_one_inequality")
    assert np.max(np.abs(ref.z - np.minimum(ref.q, 1.0))) <= 1e-9


def test_cone_formula():
    ref = pr.reference("n3_one_soc_only")
    expect = np.stack([conic._proj_cone(conic.SOC, row, 0) for row in ref.q])
    assert np.max(np.abs(ref.z - expect)) <= 1e-9
    s, t = np.linalg.norm(ref.q[:, :2], axis=1), ref.q[:, 2]
    assert np.any(s <= t) and np.any(s <= -t) and np.any((s > t) & (s > -t))          # all three regions are in the batch


# ------------------------------------------------------------------ the reference Jacobian
@pytest.mark.parametrize("name", NAMES)
def test_reference_jacobian_matches_finite_differences(name):
    cs, ref = pr.make_cs(name), pr.reference(name)
    rows = [b for b in range(pr.BATCH) if not ref.kink[b]][:3] + [b for b in range(pr.BATCH)
                                                                   if not ref.kink[b] and not ref.interior[b]][:3]
    step = 1e-5
    for b in set(rows):
        J, _ = pr.jacobian_row(cs, ref.q[b], ref.z[b])
        cols = list(range(cs.n))[:4]
        qs = np.concatenate([np.stack((ref.q[b] + step * np.eye(cs.n)[j], ref.q[b] - step * np.eye(cs.n)[j])) for j in cols])
        zs = pr.project_rows(cs, qs)
        for at, j in enumerate(cols):
            fd = (zs[2 * at] - zs[2 * at + 1]) / (2 * step)
            assert np.max(np.abs(fd - J[:, j])) <= 2e-5 * (1.0 + np.max(np.abs(J[:, j]))), (name, b, j)


@pytest.mark.parametrize("name", NAMES)
def test_kink_share_within_the_cap(name):
    ref = pr.reference(name)
    for B in pr.BATCHES:
        assert np.count_nonzero(ref.kink[:B]) <= pr.kink_cap(B), (name, B, np.count_nonzero(ref.kink[:B]))
    assert np.any(~ref.interior), name
    if name != "n32_full":
        assert np.any(ref.interior), name


# ------------------------------------------------------------------ the host mirror
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("name", NAMES)
def test_mirror_agrees_with_the_reference(name, dtype_name):
    run = pr.mirror_run(name, dtype_name)
    assert run.iters.max() < pr.MAX_ITERS, (name, run.iters.max())
    # the bars are KINK_FACTOR times the mirror's own gap: this shows the gap is at the scale of the stop tolerance times
    # the conditioning of the case, and that compare() passes on the mirror itself
    assert pr.compare(name, dtype_name, run.z, run.grad_q, run.iters, capped=False) == []
    fwd_bar, bwd_bar, _ = pr.bars(name, dtype_name, capped=False)
    assert fwd_bar <= 2e3 * pr.EPS[dtype_name] and bwd_bar <= 2e4 * pr.EPS[dtype_name], (fwd_bar, bwd_bar)


def _module(name, **kw):
    return projection.ProjectionModule(pr.make_cs(name), create_map=False, **kw)


@pytest.mark.parametrize("name", SMALL)
def test_module_forward_and_backward_on_host(name):
    cs, ref = pr.make_cs(name), pr.reference(name)
    layer = _module(name, max_iters=pr.MAX_ITERS, eps=1e-9).double()
    q = torch.from_numpy(ref.q.copy()).requires_grad_(True)
    z, iters = layer.project(q)
    (z * torch.from_numpy(ref.gy @ cs.NA_E)).sum().backward()
    assert pr.compare(name, "float64", z.detach().numpy(), q.grad.numpy(), iters.numpy()) == []
    # forward(): the same z through the affine map of the (reference-typed, fp32-born) buffers
    y = layer(q.detach())
    assert y.shape == (pr.BATCH, cs.k, 1) and torch.equal(layer.proj_iters, iters)
    assert torch.allclose(y[:, :, 0], z.detach() @ layer.NA_E.T + layer.yp.T, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["n3_box", "n3_one_soc_only", "k8_n5_ragged_equalities"])
def test_gradcheck(name):
    ref = pr.reference(name)
    layer = _module(name, max_iters=20000, eps=1e-13).double()
    rows = [b for b in range(pr.BATCH) if ref.margin[b] > 1e-2 and not ref.interior[b]][:4]
    q = torch.from_numpy(ref.q[rows]).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: layer.project(t)[0], (q,), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_modes_and_training_flag():
    name = "n3_box"
    q = torch.from_numpy(pr.reference(name).q).float()
    pp, up = _module(name, mode='PP'), _module(name, mode='UP')
    inside = torch.from_numpy(pr.reference(name).interior.copy())
    for layer in (pp, up):
        layer.train()
    y_pp_train, y_up_train = pp(q), up(q)
    assert torch.equal(y_up_train[:, :, 0], q)                       # UP in training: z = q (NA_E = I, yp = 0 here)
    assert not torch.equal(y_pp_train[~inside], y_up_train[~inside])
    for layer in (pp, up):
        layer.eval()
    assert torch.equal(pp(q), y_pp_train) and torch.equal(up(q), y_pp_train)
    assert pp.getDimAfterMap() == 3
    mapped = projection.ProjectionModule(pr.make_cs(name), input_dim=7, mode='PP')
    assert isinstance(mapped.mapper, torch.nn.Linear) and mapped(torch.randn(5, 7)).shape == (5, 3, 1)
    with pytest.raises(ValueError):
        _module(name, mode='RAYEN')


def test_buffers_and_pickle_round_trip():
    name = "k8_n5_ragged_equalities"
    layer = _module(name)
    names = {n for n, _ in layer.named_buffers()}
    assert {"A_p", "b_p", "yp", "NA_E", "z0", "y0", "all_P", "all_q", "all_r", "all_M", "all_s", "all_c", "all_d"} <= names
    q = torch.from_numpy(pr.reference(name).q).float()
    y = layer(q)
    layer._proj_packs["fake"] = object()
    clone = pickle.loads(pickle.dumps(layer))
    assert clone._proj_packs == {} and clone._constants == {}
    assert torch.equal(clone(q), y)
    assert layer.double()._constants == {}                           # .to() drops the derived constants


def test_lmi_set_raises():
    cs = workloads.build_constraints(workloads.random_lmi(4, 5, seed=1))
    with pytest.raises(NotImplementedError):
        projection.ProjectionModule(cs, create_map=False)


@pytest.mark.parametrize("name", ["n3_box", "k8_n5_ragged_equalities"])
def test_project_batch_equals_a_loop_of_project(name):
    cs = pr.make_cs(name)
    rng = np.random.default_rng(11)
    Y = (cs.y0.T + 0.7 * rng.standard_normal((6, cs.k)))          # off the equality subspace too
    out, dist = cs.projectBatch(Y)
    for b in range(Y.shape[0]):
        y, d = cs.project(Y[b])
        assert np.max(np.abs(out[b] - y[:, 0])) <= 1e-6, (name, b)
        assert abs(dist[b] - d) <= 1e-6 * (1.0 + d), (name, b)
    yt, dt = cs.projectBatch(torch.from_numpy(Y).float())
    assert yt.dtype == torch.float32 and np.max(np.abs(yt.numpy() - out)) <= 1e-4


# ------------------------------------------------------------------ the comparisons catch a wrong implementation
def _defective_run(name, dtype_name, defect):
    """tests/proj_reference.py::mirror_run on a copy of the mirror with one deliberate defect."""
    dtype = getattr(torch, dtype_name)
    cs, module = pr.make_cs(name), pr.module_for(name)
    c = module.constants(dtype, torch.device("cpu"))
    q, gy = pr.make_inputs(name)
    q, g = torch.from_numpy(q).to(dtype), torch.from_numpy(gy @ cs.NA_E).to(dtype)
    eps, limit = pr.EPS[dtype_name], 300
    h = c.h if defect != "no_h_in_the_cone_shift" else torch.zeros_like(c.h)
    sign = -1.0 if defect == "moreau_sign" else 1.0

    def derivative(v, dv):
        if defect == "soc_derivative_is_a_mask":
            p = projection.cone_project(c, v)
            return torch.where(p != 0, dv, torch.zeros_like(dv))
        return projection.cone_derivative(c, v, dv)

    def loop(rhs2, x, v, done, op, hh, w0):
        out, vstop, iters = x.clone(), v.clone(), torch.zeros(x.shape[0], dtype=torch.int32)
        for t in range(1, limit + 1):
            p = op(v)
            xt = (projection.SIGMA * x + rhs2 + w0 + c.rho * (sign * (2.0 * p - v) @ c.G)) @ c.Kinv
            r = xt @ c.G.T + hh - p
            dx = xt - x
            conv = (r.abs().amax(1) <= eps * (1 + p.abs().amax(1))) & (dx.abs().amax(1) <= eps * (1 + xt.abs().amax(1)))
            stop = ~done & (conv | (t == limit))
            out, vstop = torch.where(stop[:, None], xt, out), torch.where(stop[:, None], v, vstop)
            iters = torch.where(~done, torch.full_like(iters, t), iters)
            go = (~done & ~stop)[:, None]
            v, x = torch.where(go, v + projection.ALPHA * r, v), torch.where(go, x + projection.ALPHA * dx, x)
            done = done | stop
        return out, vstop, iters

    v_raw = q @ c.G.T + h
    p0 = projection.cone_project(c, v_raw)
    interior = (p0 == v_raw).all(1)
    z, vstar, iters = loop(2 * q, q, p0, interior, lambda v: projection.cone_project(c, v), h, c.w0)
    z = torch.where(interior[:, None], q, z)
    iters = torch.where(interior, torch.zeros_like(iters), iters)
    vstar = torch.where(interior[:, None], v_raw, vstar)
    scale = g.abs().amax(1, keepdim=True)
    gn = g / scale
    D = lambda dv: derivative(vstar, dv)                # noqa: E731
    grad, _, _ = loop(2 * gn, gn, D(gn @ c.G.T), interior, D, 0.0, 0.0)
    grad = torch.where(interior[:, None], g, grad * scale)
    return z.double().numpy(), grad.double().numpy(), iters.numpy()


def test_the_undamaged_copy_passes():
    z, grad, iters = _defective_run("k8_n5_ragged_equalities", "float32", None)
    assert pr.compare("k8_n5_ragged_equalities", "float32", z, grad, iters) == []


@pytest.mark.parametrize("defect", ["moreau_sign", "soc_derivative_is_a_mask", "no_h_in_the_cone_shift"])
def test_comparisons_catch_a_defect(defect):
    z, grad, iters = _defective_run("k8_n5_ragged_equalities", "float32", defect)
    assert pr.compare("k8_n5_ragged_equalities", "float32", z, grad, iters) != [], defect


# ------------------------------------------------------------------ served()
def test_served_rule_and_the_lds_limit():
    at, over = pr.lds_limit_rows()
    assert pr.lds_bytes(64, at, 4) <= pr.LDS_LIMIT < pr.lds_bytes(64, over, 4)
    assert pr.shape_of(pr.LDS_AT_LIMIT.name) == (64, at, 0) and pr.shape_of(pr.LDS_JUST_OVER.name) == (64, over, 0)
    assert pr.case_served("n64_c3_shape", "float32") and not pr.case_served("n64_c3_shape", "float64")
    for name in NAMES:
        assert pr.SHAPE[name] == pr.shape_of(name), name
    for name in NAMES[:-1]:
        assert pr.case_served(name, "float32") and pr.case_served(name, "float64"), name
