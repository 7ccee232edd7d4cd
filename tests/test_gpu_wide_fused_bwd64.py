"""The fp64 fused wide backward (``wide_backward='fused64'``, rayen_amd/csrc/rayen_wide_fused_bwd64.hip) on an MI355X:
against fp64 autograd through the oracle, next to the products route against a host restatement in np.longdouble, the bits
contract (a row's gradient bits depend on the set and that row's inputs alone), NaN handling, refusals, training and stream
capture.  The sets and inputs: tests/wide_fused_bwd64_cases.py."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_fused_bwd64_cases as C                             # noqa: E402
import wide_fused_cases as F                                   # noqa: E402
from rayen_amd import _lib, ops                                # noqa: E402
from rayen_amd.constraint_module import ConstraintModule       # noqa: E402
from rayen_amd.pack import DevicePack                          # noqa: E402
from test_gpu_backward import _assert_gradient, _oracle_grad   # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = torch.float64
# F of the per-row bar max(2 x the products route's error on that row, F): the PRODUCTS route's worst row error against the
# np.longdouble restatement over all cases of C.CASES, measured once on an MI355X -- 1.878e-15, on mixE (the other cases:
# 3.8e-16 to 6.8e-16; test_next_to_the_products_route_on_the_same_records prints both routes' per case).  Both routes are
# exact fp64 sums of the same terms in another order and neither order is privileged: a row of the fused route may be off by
# twice the products route's error on that row, or by F where that row's own error happens to be small.
FLOOR = 1.878e-15


def _layer(cs, dtype=F64, **kw):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return ConstraintModule(cs, create_map=False, **kw).cuda()
    finally:
        torch.set_default_dtype(prev)


_LAYERS, _PACKS, _ORACLE, _RECORDS, _REFERENCE = {}, {}, {}, {}, {}


def _module(name, wide_kernel="products"):
    key = (name, wide_kernel)
    if key not in _LAYERS:
        _LAYERS[key] = _layer(C.cs(name), wide_kernel=wide_kernel, wide_backward="fused64")
    return _LAYERS[key]


def _pack(name):
    """The device pack on which the records are made (the relaid layout where the case has one), built once."""
    if name not in _PACKS:
        _PACKS[name] = DevicePack(C.consts(name), 0)
    return _PACKS[name]


def _truth(name):
    """fp64 autograd through the oracle, computed once per case and left unchanged."""
    if name not in _ORACLE:
        _ORACLE[name] = _oracle_grad(C.cs(name), C.inputs(name).unsqueeze(2), C.grads(name))[0]
        _ORACLE[name].setflags(write=False)
    return _ORACLE[name]


def _records(name):
    """(v, kappa, active, G) on the device, from the products forward; once per case."""
    if name not in _RECORDS:
        v = C.inputs(name).cuda()
        _, kappa, active = ops.project_raw(v, _pack(name))
        assert _lib.load().rayen_last_forward_kernel() == _lib.KERNEL_PRODUCTS
        _RECORDS[name] = (v, kappa, active, C.grads(name).cuda())
    return _RECORDS[name]


def _reference(name):
    """The np.longdouble restatement on the recorded (kappa, active); once per case, left unchanged."""
    if name not in _REFERENCE:
        v, kappa, active, G = _records(name)
        _REFERENCE[name] = C.reference(C.consts(name), v.cpu().numpy(), kappa.cpu().numpy(), active.cpu().numpy(), G.cpu().numpy())
        _REFERENCE[name].setflags(write=False)
    return _REFERENCE[name]


def _fused(name, v, kappa, active, G, **kw):
    return ops.backward_raw(v, kappa, active, G, _pack(name), wide_backward="fused64", **kw)


def _row_err_long(got, want):
    got = np.asarray(got).astype(np.longdouble)
    scale = np.maximum(np.max(np.abs(want), axis=1), np.longdouble(1e-300))
    return (np.max(np.abs(got - want), axis=1) / scale).astype(np.float64)


@pytest.mark.parametrize("wide_kernel", ["products", "fused64"])
@pytest.mark.parametrize("name", C.CASES)
def test_against_fp64_autograd_through_the_oracle(name, wide_kernel):
    """Through the module, which packs every set in the packer's own layout: the relaid layouts of plan_a and plan_c (a
    cone's aux rows at 15 | 16, segments of 17 / 1 / 15 / 16 rows behind a gap) do not run here.  They run in
    test_next_to_the_products_route_on_the_same_records, against the np.longdouble restatement -- whose formula is the
    kernel's own, and which this test holds to the oracle on the same sets in the packer's layout."""
    cs, layer = C.cs(name), _module(name, wide_kernel)
    x, G = C.inputs(name).unsqueeze(2), C.grads(name)
    xg = x.cuda().requires_grad_(True)
    y = layer(xg)
    assert _lib.load().rayen_last_forward_kernel() == (_lib.KERNEL_WIDE_FUSED64 if wide_kernel == "fused64" else _lib.KERNEL_PRODUCTS)
    (y[:, :, 0] * G.cuda()).sum().backward()
    got = xg.grad[:, :, 0].cpu().numpy()
    assert np.all(np.isfinite(got)) and not layer._hip_unsupported
    assert layer._route_key() == wide_kernel + "+bwd_fused64"
    _assert_gradient(got, _truth(name), cs, x, G, F64, what=f"{name} behind {wide_kernel}")


@pytest.mark.parametrize("name", C.CASES)
def test_next_to_the_products_route_on_the_same_records(name):
    dp = _pack(name)
    v, kappa, active, G = _records(name)
    want = _reference(name)
    products = ops.backward_raw(v, kappa, active, G, dp).cpu().numpy()
    fused = _fused(name, v, kappa, active, G).cpu().numpy()
    err_p, err_f = _row_err_long(products, want), _row_err_long(fused, want)
    print(f"{name}: worst row error against the np.longdouble restatement: fused64 {err_f.max():.3e}, products {err_p.max():.3e}; "
          f"median {np.median(err_f):.3e} / {np.median(err_p):.3e}")
    assert np.all(np.isfinite(fused)) and np.all(np.isfinite(products))
    bad = ~(err_f <= np.maximum(2 * err_p, FLOOR))          # kink rows are not exempt
    assert not bad.any(), (np.flatnonzero(bad)[:5], err_f[bad][:5], err_p[bad][:5])


@pytest.mark.parametrize("name", (*C.MIXED, "k1024"))
def test_segments_no_input_activates_run_on_hand_set_records(name):
    """mixI, mixE and k1024 keep the inputs of tests/wide_fused_bwd_cases.py, under which some non-linear segments are active
    on fewer than 3 rows (the second dense quadratic and the 4-row QUAD_FAC of mixE, the 65-row cone of k1024 -- the set with
    the largest LDS plan and the only T tile next to a 1 026-word v stride -- on none).  The backward takes the recorded
    ``active`` as it is: here every non-linear segment is NAMED on six clipped rows each (interleaved, so that the first
    tiles walk all of them), and the result is held to the np.longdouble restatement on the same hand-set records under the
    bar of test_next_to_the_products_route_on_the_same_records, next to the products route."""
    c, dp = C.consts(name), _pack(name)
    v, kappa, active, G = _records(name)
    nonlin = [i for i, s in enumerate(c.segments) if s.type != _lib.SEG_LIN]
    cov = C.coverage(name)
    assert any(len(cov["rows"][i]) < 3 for i in nonlin), name            # (what this test is for)
    clipped = torch.nonzero(kappa > 1).flatten()
    per = 6
    assert len(clipped) >= per * len(nonlin)
    hand = active.clone()
    named = torch.zeros(300, dtype=torch.bool, device=DEV)
    for j, i in enumerate(nonlin):
        rows = clipped[j::len(nonlin)][:per]
        hand[rows, 0] = i
        hand[rows, 1] = 0
        named[rows] = True
    assert int(named.sum()) == per * len(nonlin)
    want = C.reference(c, v.cpu().numpy(), kappa.cpu().numpy(), hand.cpu().numpy(), G.cpu().numpy())
    products = ops.backward_raw(v, kappa, hand, G, dp).cpu().numpy()
    got = _fused(name, v, kappa, hand, G)
    fused = got.cpu().numpy()
    err_p, err_f = _row_err_long(products, want), _row_err_long(fused, want)
    rows = named.cpu().numpy()
    print(f"{name}: {len(nonlin)} non-linear segments named on {per} rows each; worst error of those rows against the "
          f"np.longdouble restatement: fused64 {err_f[rows].max():.3e}, products {err_p[rows].max():.3e}")
    assert np.all(np.isfinite(fused)) and np.all(np.isfinite(products))
    bad = ~(err_f <= np.maximum(2 * err_p, FLOOR))
    assert not bad.any(), (np.flatnonzero(bad)[:5], err_f[bad][:5], err_p[bad][:5])
    # the rows whose record was left alone keep their bits; the tile and the grouping change none
    full = _fused(name, v, kappa, active, G)
    assert torch.equal(got[~named], full[~named])
    assert torch.equal(_fused(name, v, kappa, hand, G, wide_samples=16), got)
    assert torch.equal(_fused(name, v, kappa, hand, G, group=False), got)


@pytest.mark.parametrize("name", (*C.CASES, "k1025"))
def test_the_exported_plan_is_the_restated_one(name):
    lib, dp = _lib.load(), _pack(name)
    served = int(name != "k1025")
    assert lib.rayen_wide_fused_bwd64_served(dp.handle) == served
    for samples in (0, 16, 32):
        out = np.zeros(11, dtype=np.int64)
        assert lib.rayen_wide_fused_bwd64_plan(dp.handle, samples, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == 0
        assert dict(zip(C.PLAN_KEYS, out.tolist())) == C.plan_of(dp.consts, samples), (name, samples)
    assert lib.rayen_wide_fused_bwd64_plan(dp.handle, 8, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == -1
    n_nl = sum(s.type != _lib.SEG_LIN for s in dp.consts.segments)
    assert lib.rayen_wide_fused_bwd64_workspace_bytes(dp.handle, 300) == (C.workspace(n_nl, 300) if served else 0)
    assert lib.rayen_wide_fused_bwd_served(dp.handle, 1) == 0            # 'fused' stays fp32 only


@pytest.mark.parametrize("name", C.BITS)
def test_a_rows_bits_depend_on_the_set_and_that_rows_inputs_alone(name):
    n = C.consts(name).n
    v, kappa, active, G = _records(name)
    full = _fused(name, v, kappa, active, G)
    assert full.shape == (300, n) and full.dtype == F64
    # the tile: 16 against 32 against the plan's choice
    assert torch.equal(_fused(name, v, kappa, active, G, wide_samples=16), full)
    if C.plan_of(C.consts(name), 32)["served"]:
        assert torch.equal(_fused(name, v, kappa, active, G, wide_samples=32), full)
        assert torch.equal(_fused(name, v, kappa, active, G, wide_samples=32, group=False), full)
    else:
        assert name == "s16_first"
    # grouping by active constraint against batch order; the batch flipped
    assert torch.equal(_fused(name, v, kappa, active, G, group=False), full)
    assert torch.equal(_fused(name, v, kappa, active, G, group=False, wide_samples=16), full)
    flipped = [t.flip(0).contiguous() for t in (v, kappa, active, G)]
    for group in (True, False):
        assert torch.equal(_fused(name, *flipped, group=group).flip(0), full), group
    # prefixes, an interior slice, nothing
    for B in (1, 15, 16, 17, 31, 32, 33, 300):
        assert torch.equal(_fused(name, v[:B], kappa[:B], active[:B], G[:B]), full[:B]), B
    assert torch.equal(_fused(name, v[5:70], kappa[5:70], active[5:70], G[5:70]), full[5:70])
    assert _fused(name, v[:0], kappa[:0], active[:0], G[:0]).shape == (0, n)
    # rows with a stride beyond n: what lies between them is not read
    buf = torch.full((300, n + 7), float("nan"), device=DEV, dtype=F64)
    buf[:, :n] = v
    assert torch.equal(_fused(name, buf[:, :n], kappa, active, G), full)
    # v wider than n: the extra columns of grad_v are zero
    buf = torch.full((300, n + 7), 3.0, device=DEV, dtype=F64)
    buf[:, :n] = v
    wide = _fused(name, buf, kappa, active, G)
    assert wide.shape == (300, n + 7) and torch.equal(wide[:, :n], full) and bool((wide[:, n:] == 0).all())


@pytest.mark.parametrize("name", C.MIXED)
def test_the_default_call_does_group(name):
    assert _lib.load().rayen_wide_fused_bwd64_workspace_bytes(_pack(name).handle, 300) > 0


@pytest.mark.parametrize("name", C.MIXED)
def test_a_nan_stays_in_its_row(name):
    dp = _pack(name)
    v, _, _, G = (t[:64] for t in _records(name))
    # (the records of both batches from the fp64 fused forward, whose rows do not depend on their batch-mates; the library
    # GEMM of the products forward gives no such promise)
    _, kappa, active = ops.project_raw(v, dp, wide_kernel="fused64")
    full = _fused(name, v, kappa, active, G)
    keep = torch.arange(64, device=DEV) != 17
    bad = v.clone()
    bad[17, 3] = float("nan")
    try:
        _, kb, ab = ops.project_raw(bad, dp, wide_kernel="fused64")
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
    # fp32 input
    cs = F.cs("k129")
    x = F.inputs(cs.n, 8)
    G = torch.ones(8, cs.k)
    layer = _layer(cs, torch.float32, wide_backward="fused64")
    with pytest.raises(_lib.RayenError) as err:
        _train_step(layer, x, G)
    assert err.value.code == _lib.E_UNSUPPORTED
    assert _train_step(_layer(cs, torch.float32), x, G).shape == (8, cs.n, 1)         # the default route serves it
    # n = 1025
    cs = C.cs("k1025")
    x = F.inputs(cs.n, 8).double()
    G = torch.ones(8, cs.k, dtype=F64)
    layer = _layer(cs, wide_backward="fused64")
    assert lib.rayen_wide_fused_bwd64_served(layer.device_pack(DEV)[0].handle) == 0
    with pytest.raises(_lib.RayenError) as err:
        _train_step(layer, x, G)
    assert err.value.code == _lib.E_UNSUPPORTED
    assert _train_step(_layer(cs), x, G).shape == (8, 1025, 1)
    # a forced 32 samples beyond LDS
    v, kappa, active, G = (t[:8] for t in _records("k1024"))
    with pytest.raises(_lib.RayenError) as err:
        _fused("k1024", v, kappa, active, G, wide_samples=32)
    assert err.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(_lib.RayenError) as err:
        _fused("k1024", v, kappa, active, G, wide_samples=8)
    assert err.value.code == -1                       # RAYEN_E_BAD_ARG
    assert _fused("k1024", v, kappa, active, G).shape == (8, 1024)
    assert ops.backward_raw(v, kappa, active, G, _pack("k1024")).shape == (8, 1024)


@pytest.mark.eager_detour
def test_a_refusal_is_announced_once_and_remembered_per_route(monkeypatch):
    monkeypatch.delenv("RAYEN_STRICT_HIP", raising=False)
    cs = F.cs("k129")
    x = F.inputs(cs.n, 8)
    G = torch.empty(8, cs.k).uniform_(-1, 1, generator=torch.Generator().manual_seed(4))
    layer = _layer(cs, torch.float32, wide_backward="fused64")
    assert layer._route_key() == "products+bwd_fused64"
    with pytest.warns(RuntimeWarning, match="rayen_amd: no HIP backward kernel serves"):
        got = _train_step(layer, x, G)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=r"rayen_amd:", category=RuntimeWarning)
        assert torch.equal(_train_step(layer, x, G), got)                 # remembered: no second announcement
    refused = layer.device_pack(DEV)[0].__dict__["_refused_bwd"]
    assert (torch.float32, "fused64") in refused and (torch.float32, "fused") not in refused
    want = _train_step(_layer(cs, torch.float32), x, G)
    assert float((got - want).abs().max()) <= 2e-4 * max(1.0, float(want.abs().max()))


def test_training_through_both_fp64_fused_kernels():
    cs = C.cs("mixI")
    layer = _module("mixI", "fused64")
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(5)
    net = torch.nn.Linear(12, cs.n).double().cuda()
    with torch.no_grad():
        net.weight.mul_(4.0)                          # most rows start outside the set
    x = torch.empty(64, 12, dtype=F64).uniform_(-1, 1, generator=gen).cuda()
    with torch.no_grad():
        target = layer(torch.empty(64, cs.n, 1, dtype=F64).uniform_(-0.4, 0.4, generator=gen).cuda())
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        y = layer(net(x).unsqueeze(2))
        assert _lib.load().rayen_last_forward_kernel() == _lib.KERNEL_WIDE_FUSED64
        loss = ((y - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert not layer._hip_unsupported
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
