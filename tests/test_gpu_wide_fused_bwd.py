"""The fused wide backward (``wide_backward='fused'``, rayen_amd/csrc/rayen_wide_fused_bwd.hip) on an MI355X: against fp64
autograd through the oracle, next to the products route, its geometry, the grouping by active constraint, NaN handling,
refusals, training and stream capture.  The sets and inputs: tests/wide_fused_bwd_cases.py."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_fused_bwd_cases as C                               # noqa: E402
import wide_fused_cases as F                                   # noqa: E402
from rayen_amd import _lib, ops                                # noqa: E402
from rayen_amd.constraint_module import ConstraintModule       # noqa: E402
from test_gpu_backward import GRAD_TOL, _assert_gradient, _oracle_grad, _row_err   # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _layer(cs, dtype=torch.float32, **kw):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return ConstraintModule(cs, create_map=False, **kw).cuda()
    finally:
        torch.set_default_dtype(prev)


_LAYERS, _ORACLE, _RECORDS = {}, {}, {}


def _module(name, wide_kernel="products"):
    key = (name, wide_kernel)
    if key not in _LAYERS:
        _LAYERS[key] = _layer(C.cs(name), wide_kernel=wide_kernel, wide_backward="fused")
    return _LAYERS[key]


def _pack(name):
    return _module(name).device_pack(DEV)[0]


def _truth(name):
    """fp64 autograd through the oracle, computed once per case and left unchanged."""
    if name not in _ORACLE:
        _ORACLE[name] = _oracle_grad(C.cs(name), C.inputs(name), C.grads(name))[0]
    return _ORACLE[name]


def _records(name):
    """(v, kappa, active, G) on the device, from the products forward; once per case."""
    if name not in _RECORDS:
        v = C.inputs(name)[:, :, 0].cuda()
        _, kappa, active = ops.project_raw(v, _pack(name))
        _RECORDS[name] = (v, kappa, active, C.grads(name).cuda())
    return _RECORDS[name]


def _fused(name, v, kappa, active, G, **kw):
    return ops.backward_raw(v, kappa, active, G, _pack(name), wide_backward="fused", **kw)


@pytest.mark.parametrize("wide_kernel", ["products", "fused"])
@pytest.mark.parametrize("name", C.CASES)
def test_against_fp64_autograd_through_the_oracle(name, wide_kernel):
    cs, layer = C.cs(name), _module(name, wide_kernel)
    x, G = C.inputs(name), C.grads(name)
    xg = x.cuda().requires_grad_(True)
    y = layer(xg)
    assert _lib.load().rayen_last_forward_kernel() == (_lib.KERNEL_WIDE_FUSED if wide_kernel == "fused" else _lib.KERNEL_PRODUCTS)
    (y[:, :, 0] * G.cuda()).sum().backward()
    got = xg.grad[:, :, 0].cpu().double().numpy()
    assert np.all(np.isfinite(got)) and not layer._hip_unsupported
    _assert_gradient(got, _truth(name), cs, x, G, torch.float32, what=f"{name} behind {wide_kernel}")


@pytest.mark.parametrize("name", C.CASES)
def test_next_to_the_products_route_on_the_same_records(name):
    dp = _pack(name)
    v, kappa, active, G = _records(name)
    _, k64, a64 = ops.project_raw(v.double(), dp)
    want = ops.backward_raw(v.double(), k64, a64, G.double(), dp).cpu().numpy()
    products = ops.backward_raw(v, kappa, active, G, dp).double().cpu().numpy()
    fused = _fused(name, v, kappa, active, G).double().cpu().numpy()
    err_p, err_f = _row_err(products, want), _row_err(fused, want)
    print(f"{name}: worst row error against fp64: fused {err_f.max():.3e}, products {err_p.max():.3e}; "
          f"median {np.median(err_f):.3e} / {np.median(err_p):.3e}")
    assert np.all(np.isfinite(fused))
    bad = ~(err_f <= np.maximum(2 * err_p, GRAD_TOL[torch.float32]))          # kink rows are not exempt
    assert not bad.any(), (np.flatnonzero(bad)[:5], err_f[bad][:5], err_p[bad][:5])


@pytest.mark.parametrize("name", ["mixI", "mixE"])
def test_geometry(name):
    n = C.cs(name).n
    v, kappa, active, G = _records(name)
    full = _fused(name, v, kappa, active, G)
    assert full.shape == (300, n)
    for B in (1, 31, 32, 33, 300):
        assert torch.equal(_fused(name, v[:B], kappa[:B], active[:B], G[:B]), full[:B]), B
    assert torch.equal(_fused(name, v[5:70], kappa[5:70], active[5:70], G[5:70]), full[5:70])
    assert _fused(name, v[:0], kappa[:0], active[:0], G[:0]).shape == (0, n)
    # rows with a stride beyond n: what lies between them is not read
    buf = torch.full((300, n + 7), float("nan"), device=DEV)
    buf[:, :n] = v
    assert torch.equal(_fused(name, buf[:, :n], kappa, active, G), full)
    # v wider than n: the extra columns of grad_v are zero
    buf = torch.full((300, n + 7), 3.0, device=DEV)
    buf[:, :n] = v
    wide = _fused(name, buf, kappa, active, G)
    assert wide.shape == (300, n + 7) and torch.equal(wide[:, :n], full) and bool((wide[:, n:] == 0).all())


@pytest.mark.parametrize("name", ["mixI", "mixE"])
def test_grouping_changes_no_bit(name):
    v, kappa, active, G = _records(name)
    assert _lib.load().rayen_wide_fused_bwd_workspace_bytes(_pack(name).handle, 300) > 0       # (the default does group)
    full = _fused(name, v, kappa, active, G)
    assert torch.equal(_fused(name, v, kappa, active, G, group=False), full)
    back = _fused(name, v.flip(0).contiguous(), kappa.flip(0).contiguous(), active.flip(0).contiguous(), G.flip(0).contiguous())
    assert torch.equal(back.flip(0), full)
    back = _fused(name, v.flip(0).contiguous(), kappa.flip(0).contiguous(), active.flip(0).contiguous(), G.flip(0).contiguous(),
                  group=False)
    assert torch.equal(back.flip(0), full)


@pytest.mark.parametrize("name", ["mixI", "mixE"])
def test_a_nan_stays_in_its_row(name):
    dp = _pack(name)
    v, kappa, active, G = (t[:64] for t in _records(name))
    full = _fused(name, v, kappa, active, G)
    keep = torch.arange(64, device=DEV) != 17
    bad = v.clone()
    bad[17, 3] = float("nan")
    try:
        _, kb, ab = ops.project_raw(bad, dp)
    finally:
        dp.nan_flag.zero_()
    assert bool(torch.isnan(kb[17])) and torch.equal(kb[keep], kappa[keep]) and torch.equal(ab[keep], active[keep])
    for group in (True, False):
        got = _fused(name, bad, kb, ab, G, group=group)
        assert torch.equal(got[keep], full[keep]), group          # rows 16 and 18 among them
        Gb = G.clone()
        Gb[17, 5] = float("nan")
        got = _fused(name, v, kappa, active, Gb, group=group)
        assert torch.equal(got[keep], full[keep]) and bool(torch.isnan(got[17]).any()), group


def _train_step(layer, x, G):
    xg = x.cuda().requires_grad_(True)
    (layer(xg)[:, :, 0] * G.cuda()).sum().backward()
    return xg.grad


def test_refusals_are_errors_under_strict_mode():
    assert os.environ.get("RAYEN_STRICT_HIP") == "1"
    lib = _lib.load()
    # fp64 input
    cs = F.cs("k129")
    x = F.inputs(cs.n, 8).double()
    G = torch.ones(8, cs.k, dtype=torch.float64)
    layer = _layer(cs, torch.float64, wide_backward="fused")
    with pytest.raises(_lib.RayenError) as err:
        _train_step(layer, x, G)
    assert err.value.code == _lib.E_UNSUPPORTED
    assert lib.rayen_wide_fused_bwd_served(layer.device_pack(DEV)[0].handle, 1) == 0
    assert lib.rayen_wide_fused_bwd_served(layer.device_pack(DEV)[0].handle, 0) == 1
    assert _train_step(_layer(cs, torch.float64), x, G).shape == (8, cs.n, 1)         # the default route serves it
    # n = 1025
    cs = F.cs("k1025")
    x = F.inputs(cs.n, 8)
    G = torch.ones(8, cs.k)
    layer = _layer(cs, wide_backward="fused")
    assert lib.rayen_wide_fused_bwd_served(layer.device_pack(DEV)[0].handle, 0) == 0
    with pytest.raises(_lib.RayenError) as err:
        _train_step(layer, x, G)
    assert err.value.code == _lib.E_UNSUPPORTED
    assert _train_step(_layer(cs), x, G).shape == (8, 1025, 1)


@pytest.mark.eager_detour
def test_a_refusal_is_announced_once_and_remembered_per_route(monkeypatch):
    monkeypatch.delenv("RAYEN_STRICT_HIP", raising=False)
    cs = F.cs("k129")
    x = F.inputs(cs.n, 8).double()
    G = torch.empty(8, cs.k, dtype=torch.float64).uniform_(-1, 1, generator=torch.Generator().manual_seed(4))
    layer = _layer(cs, torch.float64, wide_backward="fused")
    assert layer._route_key() == "products+bwd_fused"
    with pytest.warns(RuntimeWarning, match="rayen_amd: no HIP backward kernel serves"):
        got = _train_step(layer, x, G)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=r"rayen_amd:", category=RuntimeWarning)
        assert torch.equal(_train_step(layer, x, G), got)                 # remembered: no second announcement
    assert (torch.float64, "fused") in layer.device_pack(DEV)[0].__dict__["_refused_bwd"]
    want = _train_step(_layer(cs, torch.float64), x, G)
    assert float((got - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))


def test_training_through_both_fused_kernels():
    cs = C.cs("mixI")
    layer = _module("mixI", "fused")
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(5)
    net = torch.nn.Linear(12, cs.n).cuda()
    with torch.no_grad():
        net.weight.mul_(4.0)                          # most rows start outside the set
    x = torch.empty(64, 12).uniform_(-1, 1, generator=gen).cuda()
    with torch.no_grad():
        target = layer(torch.empty(64, cs.n, 1).uniform_(-0.4, 0.4, generator=gen).cuda())
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        y = layer(net(x).unsqueeze(2))
        assert _lib.load().rayen_last_forward_kernel() == _lib.KERNEL_WIDE_FUSED
        loss = ((y - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert np.all(np.isfinite(losses)) and all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert losses[-1] < losses[0], losses


def test_a_capture_after_one_warm_call_replays_to_the_eager_result():
    name = "mixE"
    v, kappa, active, G = _records(name)
    eager = _fused(name, v, kappa, active, G)            # the warm call: the images exist from here on
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _fused(name, v, kappa, active, G)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
