"""The fused wide forward (``wide_kernel='fused'``, rayen_amd/csrc/rayen_wide_fused.hip) on an MI355X: against the oracle,
against fp64 on the same pack next to the products route, its geometry, NaN handling, training and refusals.  The sets and
inputs: tests/wide_fused_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_fused_cases as C                                   # noqa: E402
from helpers import rel_err_rows                               # noqa: E402
from oracle import rayen_oracle as oracle                      # noqa: E402
from rayen_amd import _lib, ops, workloads                     # noqa: E402
from rayen_amd.constraint_module import ConstraintModule       # noqa: E402
from test_gpu_backward import _assert_gradient, _oracle_grad   # noqa: E402
from test_gpu_parity import FP32_TOL, VIOLATION_TOL, _oracle_forward   # noqa: E402
from wide_fused_bwd_cases import assert_active_names_a_maximiser   # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _layer(cs, dtype=torch.float32, **kw):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return ConstraintModule(cs, create_map=False, **kw).cuda()
    finally:
        torch.set_default_dtype(prev)


_LAYERS = {}


def _fused(name):
    """(cs, module with wide_kernel='fused', its device pack), built once per case."""
    if name not in _LAYERS:
        cs = C.cs(name)
        layer = _layer(cs, wide_kernel="fused")
        _LAYERS[name] = (cs, layer, layer.device_pack(DEV)[0])
    return _LAYERS[name]


def _last_kernel():
    return _lib.load().rayen_last_forward_kernel()


@pytest.mark.parametrize("name", C.CASES)
def test_against_the_oracle(name):
    cs, layer, dp = _fused(name)
    x = C.inputs(cs.n)
    y = layer(x.cuda()).cpu().numpy()[:, :, 0]
    assert _last_kernel() == _lib.KERNEL_WIDE_FUSED and not layer._hip_unsupported
    y_ref = _oracle_forward(cs, x, torch.float32)
    err = rel_err_rows(y, y_ref)
    print(f"{name}: worst row error against the oracle {err.max():.3e} (bar {FP32_TOL:.0e})")
    assert np.max(err) <= FP32_TOL
    raw = C.raw(name)
    ours, theirs = oracle.max_violation(raw, y), oracle.max_violation(raw, y_ref)
    print(f"{name}: violation {ours:.3e}, the oracle's own {theirs:.3e}")
    assert ours <= max(VIOLATION_TOL, 3 * theirs)
    assert np.array_equal(y[8], dp.consts.y0.astype(np.float32))          # the zero direction returns y0


@pytest.mark.parametrize("name", C.CASES)
def test_kappa_and_active_against_fp64_on_the_same_pack(name):
    cs, layer, dp = _fused(name)
    v = C.inputs(cs.n)[:, :, 0].cuda()
    _, k64, _ = ops.project_raw(v.double(), dp)
    _, kp, _ = ops.project_raw(v, dp)
    assert _last_kernel() == _lib.KERNEL_PRODUCTS
    _, kf, af = ops.project_raw(v, dp, wide_kernel="fused")
    assert _last_kernel() == _lib.KERNEL_WIDE_FUSED
    k64 = k64.cpu().numpy()
    err_f = np.abs(kf.double().cpu().numpy() - k64)
    err_p = np.abs(kp.double().cpu().numpy() - k64)
    scale = np.maximum(1.0, k64)
    print(f"{name}: kappa error / max(1, kappa64): fused {np.max(err_f / scale):.3e}, products {np.max(err_p / scale):.3e}")
    assert np.all(err_f <= np.maximum(2 * err_p, 1e-5 * scale))
    # the constraint `active` names is a maximiser in fp64 (near-ties may pick another row than the products route)
    assert_active_names_a_maximiser(dp.consts, v.double().cpu().numpy(), k64, af.cpu().numpy())


@pytest.mark.parametrize("name", ["k129", "k190_n160"])
def test_geometry(name):
    cs, layer, dp = _fused(name)
    n, k = cs.n, cs.k
    v = C.inputs(n)[:, :, 0].cuda()
    y, kappa, active = ops.project_raw(v, dp, wide_kernel="fused")
    for B in (1, 31, 32, 33, 300):
        yb, kb, ab = ops.project_raw(v[:B], dp, wide_kernel="fused")
        assert torch.equal(yb, y[:B]) and torch.equal(kb, kappa[:B]) and torch.equal(ab, active[:B]), B
        assert torch.equal(layer(v[:B].unsqueeze(2))[:, :, 0], y[:B]), B           # the module's inference shortcut
    ys, ks, as_ = ops.project_raw(v[5:70], dp, wide_kernel="fused")
    assert torch.equal(ys, y[5:70]) and torch.equal(ks, kappa[5:70]) and torch.equal(as_, active[5:70])
    y0, k0, a0 = ops.project_raw(v[:0], dp, wide_kernel="fused")
    assert y0.shape == (0, k) and k0.shape == (0,) and a0.shape == (0, 2)
    assert layer(v[:0].unsqueeze(2)).shape == (0, k, 1)
    # rows with a stride beyond n (what lies between them is not read) and an output slice with a stride beyond k
    wide = torch.full((300, n + 7), float("nan"), device=DEV)
    wide[:, :n] = v
    yw, kw, aw = ops.project_raw(wide[:, :n], dp, wide_kernel="fused")
    assert torch.equal(yw, y) and torch.equal(kw, kappa) and torch.equal(aw, active)
    buf = torch.full((300, k + 5), -7.0, device=DEV)
    yo, _, _ = ops.project_raw(v, dp, out=buf, wide_kernel="fused")
    assert yo is buf and torch.equal(buf[:, :k], y) and bool((buf[:, k:] == -7.0).all())
    # each output alone left out
    yn, kn, an = ops.project_raw(v, dp, want_y=False, wide_kernel="fused")
    assert yn is None and torch.equal(kn, kappa) and torch.equal(an, active)
    yn, kn, an = ops.project_raw(v, dp, want_kappa=False, wide_kernel="fused")
    assert kn is None and torch.equal(yn, y) and torch.equal(an, active)
    yn, kn, an = ops.project_raw(v, dp, want_active=False, wide_kernel="fused")
    assert an is None and torch.equal(yn, y) and torch.equal(kn, kappa)
    assert _last_kernel() == _lib.KERNEL_WIDE_FUSED
    assert torch.equal(layer.computeKappa(v.unsqueeze(2)).reshape(-1), kappa)
    assert int(dp.nan_flag.item()) == 0


@pytest.mark.parametrize("name", ["k129", "k190_n160"])
def test_a_nan_stays_in_its_row(name):
    cs, layer, dp = _fused(name)
    v = C.inputs(cs.n, 64)[:, :, 0].cuda()
    y, kappa, _ = ops.project_raw(v, dp, wide_kernel="fused")
    assert int(dp.nan_flag.item()) == 0
    bad = v.clone()
    bad[17, 3] = float("nan")
    try:
        yb, kb, _ = ops.project_raw(bad, dp, wide_kernel="fused")
        assert int(dp.nan_flag.item()) == 1
    finally:
        dp.nan_flag.zero_()
    assert bool(torch.isnan(yb[17]).all()) and bool(torch.isnan(kb[17]))
    keep = torch.arange(64, device=DEV) != 17
    assert torch.equal(yb[keep], y[keep]) and torch.equal(kb[keep], kappa[keep])          # rows 16 and 18 among them
    with pytest.raises(AssertionError):
        layer(bad.unsqueeze(2))
    assert int(dp.nan_flag.item()) == 0


def test_training_through_the_fused_forward():
    """Both routes against fp64 autograd through the oracle under the rule of tests/test_gpu_backward.py; the backward is
    the products route's either way and consumes the forward's kappa and active."""
    name = "k190_n160"
    cs = C.cs(name)
    B = 64
    gen = torch.Generator().manual_seed(77)
    x = torch.empty(B, cs.n, 1).uniform_(-1, 1, generator=gen)
    x[:8] *= 1e-3
    G = torch.empty(B, cs.k).uniform_(-1, 1, generator=gen)
    want, _ = _oracle_grad(cs, x, G)
    for wide_kernel, kernel in (("fused", _lib.KERNEL_WIDE_FUSED), ("products", _lib.KERNEL_PRODUCTS)):
        layer = _fused(name)[1] if wide_kernel == "fused" else _layer(cs)
        xg = x.cuda().requires_grad_(True)
        y = layer(xg)
        assert _last_kernel() == kernel
        (y[:, :, 0] * G.cuda()).sum().backward()
        got = xg.grad[:, :, 0].cpu().double().numpy()
        assert np.all(np.isfinite(got))
        _assert_gradient(got, want, cs, x, G, torch.float32, what=wide_kernel)


def test_refusals_are_errors_under_strict_mode():
    assert os.environ.get("RAYEN_STRICT_HIP") == "1"
    # fp64 input
    cs = C.cs("k129")
    layer = _layer(cs, torch.float64, wide_kernel="fused")
    with pytest.raises(_lib.RayenError) as err:
        layer(C.inputs(cs.n, 8).double().cuda())
    assert err.value.code == _lib.E_UNSUPPORTED
    assert _lib.load().rayen_wide_fused_served(layer.device_pack(DEV)[0].handle, 1) == 0
    # n = 1025
    cs = C.cs("k1025")
    assert cs.n == 1025
    layer = _layer(cs, wide_kernel="fused")
    assert _lib.load().rayen_wide_fused_served(layer.device_pack(DEV)[0].handle, 0) == 0
    with pytest.raises(_lib.RayenError) as err:
        layer(C.inputs(cs.n, 8).cuda())
    assert err.value.code == _lib.E_UNSUPPORTED
    assert _layer(cs)(C.inputs(cs.n, 8).cuda()).shape == (8, 1025, 1)           # the default route serves it
    # a set with an LMI that the products route serves
    cs = workloads.build_constraints(workloads.random_lmi(k=40, r=50, seed=5))
    layer = _layer(cs, wide_kernel="fused")
    dp = layer.device_pack(DEV)[0]
    assert dp.products_matrix(torch.float32) is not None and _lib.load().rayen_wide_fused_served(dp.handle, 0) == 0
    x = torch.empty(8, cs.n, 1).uniform_(-1, 1, generator=torch.Generator().manual_seed(2)).cuda()
    with pytest.raises(_lib.RayenError) as err:
        layer(x)
    assert err.value.code == _lib.E_UNSUPPORTED


@pytest.mark.eager_detour
def test_a_refusal_is_announced_once_and_remembered_per_route(monkeypatch):
    monkeypatch.delenv("RAYEN_STRICT_HIP", raising=False)
    cs = C.cs("k129")
    layer = _layer(cs, torch.float64, wide_kernel="fused")
    x = C.inputs(cs.n, 8).double().cuda()
    with pytest.warns(RuntimeWarning, match="rayen_amd: no HIP kernel serves"):
        y = layer(x)
    assert layer._refused(x[:, :, 0]) and (0, torch.float64, "fused") in layer.__dict__["_unsupported"]
    import warnings
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=r"rayen_amd:", category=RuntimeWarning)
        assert torch.equal(layer(x), y)                       # remembered: no second announcement
    want = _layer(cs, torch.float64)(x)
    assert float((y - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))


def test_narrow_sets_run_what_they_ran():
    """Config 2 (n = 16) does not take the wide route: the keyword has no effect, bit for bit."""
    cs = workloads.build_constraints(workloads.make_raw("c2", seed=0))
    assert cs.n == 16
    x = torch.empty(300, cs.n, 1).uniform_(-1, 1, generator=torch.Generator().manual_seed(12)).cuda()
    y_default = _layer(cs)(x)
    kernel = _last_kernel()
    y_fused = _layer(cs, wide_kernel="fused")(x)
    assert _last_kernel() == kernel != _lib.KERNEL_WIDE_FUSED
    assert torch.equal(y_fused, y_default)
    xg = x.clone().requires_grad_(True)
    assert torch.equal(_layer(cs, wide_kernel="fused")(xg), y_default)             # the op path
