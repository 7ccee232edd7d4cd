"""The fp64 fused wide forward (``wide_kernel='fused64'``, rayen_amd/csrc/rayen_wide_fused64.hip) on an MI355X: against fp64
on the host next to the products route, the bits of a row, geometry, NaN handling, training, refusals, the calls it must not
touch, and stream capture.  The sets and inputs: tests/wide_fused64_cases.py and tests/wide_sweep_cases.py."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_fused64_cases as C                                 # noqa: E402
import wide_fused_cases as F                                   # noqa: E402
import wide_sweep_cases as WS                                  # noqa: E402
from helpers import rel_err_rows                               # noqa: E402
from rayen_amd import _lib, ops, workloads                     # noqa: E402
from rayen_amd.constraint_module import ConstraintModule       # noqa: E402
from rayen_amd.pack import DevicePack                          # noqa: E402
from test_gpu_backward import _assert_gradient, _oracle_grad   # noqa: E402
from test_gpu_parity import FP32_TOL, FP64_TOL                           # noqa: E402
from wide_fused_bwd_cases import assert_active_names_a_maximiser   # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KAPPA_TOL = 1e-9          # of max(1, kappa64)
SWEEP = tuple("sweep:" + name for name in WS.CASES)


def _layer(cs, dtype=torch.float64, **kw):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return ConstraintModule(cs, create_map=False, **kw).cuda()
    finally:
        torch.set_default_dtype(prev)


_PACKS, _LAYERS = {}, {}


def _consts(name):
    return WS.consts(name[6:]) if name.startswith("sweep:") else C.consts(name)


def _pack(name):
    """The device pack of a case (its relaid layout where it has one), built once."""
    if name not in _PACKS:
        _PACKS[name] = DevicePack(_consts(name), 0)
    return _PACKS[name]


def _inputs(name, batch=C.B):
    x = WS.inputs(name[6:])[:batch, :, 0].double() if name.startswith("sweep:") else C.inputs(name, batch)
    return x.cuda()


def _truth(name):
    return WS.truth(name[6:])[:3] if name.startswith("sweep:") else C.truth(name)


def _module(name):
    """(cs, module with wide_kernel='fused64', its device pack) of a case in the packer's layout, built once."""
    if name not in _LAYERS:
        cs = C.cs(name)
        layer = _layer(cs, wide_kernel="fused64")
        _LAYERS[name] = (cs, layer, layer.device_pack(DEV)[0])
    return _LAYERS[name]


def _run(v, dp, **kw):
    out = ops.project_raw(v, dp, wide_kernel="fused64", **kw)
    assert _last_kernel() == _lib.KERNEL_WIDE_FUSED64
    return out


def _last_kernel():
    return _lib.load().rayen_last_forward_kernel()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


WORST = {}


# ---------------------------------------------------------------- 1. against fp64 on the host
@pytest.mark.parametrize("name", (*C.CASES, *SWEEP))
def test_against_fp64_on_the_host(name):
    dp, v = _pack(name), _inputs(name)
    y64, k64, _ = _truth(name)
    y, kappa, active = _run(v, dp)
    yp, kp, _ = ops.project_raw(v, dp)
    assert _last_kernel() == _lib.KERNEL_PRODUCTS
    scale = np.maximum(1.0, k64)
    ek, ekp = np.abs(kappa.cpu().numpy() - k64) / scale, np.abs(kp.cpu().numpy() - k64) / scale
    ey, eyp = rel_err_rows(y.cpu().numpy(), y64), rel_err_rows(yp.cpu().numpy(), y64)
    WORST[name] = (float(ek.max()), float(ey.max()))
    print(f"{name}: kappa error / max(1, kappa64): fused64 {ek.max():.3e}, products {ekp.max():.3e} (bar {KAPPA_TOL:.0e}); "
          f"worst row error of y: fused64 {ey.max():.3e}, products {eyp.max():.3e} (bar {FP64_TOL:.0e})")
    assert np.all(ek <= KAPPA_TOL)
    assert np.max(ey) <= FP64_TOL
    assert_active_names_a_maximiser(dp.consts, v.cpu().numpy(), k64, active.cpu().numpy())
    assert np.array_equal(y[8].cpu().numpy(), dp.consts.y0)          # the zero direction returns y0, bit for bit
    assert int(dp.nan_flag.item()) == 0


# ---------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("name", C.CASES)
def test_a_rows_bits_depend_on_the_set_and_the_row_alone(name):
    dp, v = _pack(name), _inputs(name)
    full = _run(v, dp)
    for B in (1, 15, 16, 17, 31, 32, 33, 97):
        assert _same(_run(v[:B], dp), [t[:B] for t in full]), B
    assert _same(_run(v[5:70], dp), [t[5:70] for t in full])
    assert _same(_run(v.flip(0).contiguous(), dp), [t.flip(0) for t in full])
    lib, plan = _lib.load(), (np.zeros(13, dtype=np.int64), np.zeros(13, dtype=np.int64))
    for out, samples in zip(plan, (16, 32)):
        assert lib.rayen_wide_fused64_plan(dp.handle, samples, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == 0
        assert dict(zip(C.PLAN_KEYS, out.tolist())) == C.plan_of(dp.consts, samples)[0]
    assert plan[0][12] == 1
    if plan[1][12] == 1:           # both tiles serve the set: the same bits
        assert _same(_run(v, dp, wide_samples=16), full) and _same(_run(v, dp, wide_samples=32), full)
    else:
        assert name in ("s16_first", "k1024") and _same(_run(v, dp, wide_samples=16), full)


def test_rows_of_no_segment_change_no_bit():
    dp, v = _pack("plan_d"), _inputs("plan_d")
    zero = DevicePack(WS.zero_gaps(C.consts("plan_d")), 0)
    for samples in (16, 32):
        assert _same(_run(v, dp, wide_samples=samples), _run(v, zero, wide_samples=samples))


@pytest.mark.parametrize("relaid,plain", [("plan_e", "plan_e_plain"), ("plan_e_cut", "plan_e_plain"), ("plan_b5", None)])
def test_where_a_linear_row_sets_kappa_its_place_does_not_matter(relaid, plain):
    v = _inputs(relaid)
    _, kr, ar = _run(v, _pack(relaid))
    packer = DevicePack(C.consts(plain) if plain else C.packed(relaid), 0)
    _, kq, aq = _run(v, packer)
    lin_r = np.array([_consts(relaid).segments[s].type == _lib.SEG_LIN if s >= 0 else False for s in ar[:, 0].tolist()])
    lin_q = np.array([packer.consts.segments[s].type == _lib.SEG_LIN if s >= 0 else False for s in aq[:, 0].tolist()])
    assert np.array_equal(lin_r, lin_q) and lin_r.sum() >= 20
    # (a sum over a segment's rows is folded block by block: only where ONE row sets kappa its place cannot matter)
    lin = torch.as_tensor(lin_r, device=DEV)
    assert torch.equal(kr[lin], kq[lin])


@pytest.mark.parametrize("name", ["plan_e", "plan_e_cut"])
def test_an_exact_tie_goes_to_the_lower_row_and_the_earlier_segment(name):
    c = C.consts(name)
    _, _, active = _run(_inputs(name), _pack(name))
    active = active.cpu().numpy()
    rows = np.array([r if s >= 0 and c.segments[s].type == _lib.SEG_LIN else -1 for s, r in active])       # rows of W
    for lo, hi in ((40, 45), (104, 142), (7, 76)):
        assert np.array_equal(c.W[lo], c.W[hi])
        assert (rows == lo).sum() >= 5 and (rows == hi).sum() == 0, (lo, hi, (rows == lo).sum(), (rows == hi).sum())
    if name == "plan_e_cut":              # pair (7, 76) lies across the cut: segment 0 wins
        assert set(active[rows == 7, 0].tolist()) == {0}


# ---------------------------------------------------------------- 3. geometry and NaN
@pytest.mark.parametrize("name", ["n65", "k190_n160"])
def test_geometry(name):
    cs, layer, dp = _module(name)
    n, k = cs.n, cs.k
    v = _inputs(name, 300)
    y, kappa, active = _run(v, dp)
    for B in (1, 33, 300):
        assert torch.equal(layer(v[:B].unsqueeze(2))[:, :, 0], y[:B]), B           # the module's inference shortcut
        assert _last_kernel() == _lib.KERNEL_WIDE_FUSED64
    y0, k0, a0 = ops.project_raw(v[:0], dp, wide_kernel="fused64")
    assert y0.shape == (0, k) and k0.shape == (0,) and a0.shape == (0, 2)
    assert layer(v[:0].unsqueeze(2)).shape == (0, k, 1)
    # rows with a stride beyond n (what lies between them is not read) and an output slice with a stride beyond k
    wide = torch.full((300, n + 7), float("nan"), device=DEV, dtype=torch.float64)
    wide[:, :n] = v
    assert _same(_run(wide[:, :n], dp), (y, kappa, active))
    buf = torch.full((300, k + 5), -7.0, device=DEV, dtype=torch.float64)
    yo, _, _ = _run(v, dp, out=buf)
    assert yo is buf and torch.equal(buf[:, :k], y) and bool((buf[:, k:] == -7.0).all())
    # each output alone left out
    yn, kn, an = _run(v, dp, want_y=False)
    assert yn is None and torch.equal(kn, kappa) and torch.equal(an, active)
    yn, kn, an = _run(v, dp, want_kappa=False)
    assert kn is None and torch.equal(yn, y) and torch.equal(an, active)
    yn, kn, an = _run(v, dp, want_active=False)
    assert an is None and torch.equal(yn, y) and torch.equal(kn, kappa)
    assert torch.equal(layer.computeKappa(v.unsqueeze(2)).reshape(-1), kappa)
    assert _last_kernel() == _lib.KERNEL_WIDE_FUSED64
    assert int(dp.nan_flag.item()) == 0


@pytest.mark.parametrize("name", ["n65", "k190_n160"])
def test_a_nan_stays_in_its_row(name):
    cs, layer, dp = _module(name)
    v = _inputs(name, 64)
    y, kappa, _ = _run(v, dp)
    assert int(dp.nan_flag.item()) == 0
    bad = v.clone()
    bad[17, 3] = float("nan")
    try:
        yb, kb, _ = _run(bad, dp)
        assert int(dp.nan_flag.item()) == 1
    finally:
        dp.nan_flag.zero_()
    assert bool(torch.isnan(yb[17]).all()) and bool(torch.isnan(kb[17]))
    keep = torch.arange(64, device=DEV) != 17
    assert torch.equal(yb[keep], y[keep]) and torch.equal(kb[keep], kappa[keep])          # rows 16 and 18 among them
    with pytest.raises(AssertionError):
        layer(bad.unsqueeze(2))
    assert int(dp.nan_flag.item()) == 0


# ---------------------------------------------------------------- 4. training
def test_training_through_the_fused64_forward():
    """Against fp64 autograd through the oracle under the rule of tests/test_gpu_backward.py; the backward is the products
    route's and consumes this forward's kappa and active."""
    name = "k190_n160"
    cs, layer, _ = _module(name)
    B = 64
    gen = torch.Generator().manual_seed(77)
    x = torch.empty(B, cs.n, 1, dtype=torch.float64).uniform_(-1, 1, generator=gen)
    x[:8] *= 1e-3
    G = torch.empty(B, cs.k, dtype=torch.float64).uniform_(-1, 1, generator=gen)
    want, _ = _oracle_grad(cs, x, G)
    xg = x.cuda().requires_grad_(True)
    y = layer(xg)
    assert _last_kernel() == _lib.KERNEL_WIDE_FUSED64 and not layer._hip_unsupported
    (y[:, :, 0] * G.cuda()).sum().backward()
    got = xg.grad[:, :, 0].cpu().numpy()
    assert np.all(np.isfinite(got))
    _assert_gradient(got, want, cs, x, G, torch.float64, what="fused64")


# ---------------------------------------------------------------- 5. refusals
def _refused(fn):
    with pytest.raises(_lib.RayenError) as err:
        fn()
    return err.value.code


def test_refusals_are_errors_under_strict_mode():
    assert os.environ.get("RAYEN_STRICT_HIP") == "1"
    lib = _lib.load()
    # fp32 input (on a set that takes the wide route in fp32 too)
    cs = F.cs("k129")
    layer = _layer(cs, torch.float32, wide_kernel="fused64")
    assert _refused(lambda: layer(F.inputs(cs.n, 8).cuda())) == _lib.E_UNSUPPORTED
    # n = 1025
    cs = C.cs("k1025")
    assert cs.n == 1025
    layer = _layer(cs, wide_kernel="fused64")
    assert lib.rayen_wide_fused64_served(layer.device_pack(DEV)[0].handle) == 0
    x = F.inputs(cs.n, 8).double().cuda()
    assert _refused(lambda: layer(x)) == _lib.E_UNSUPPORTED
    assert _layer(cs)(x).shape == (8, 1025, 1)                       # the default route serves it
    # a set with an LMI that the products route serves
    cs = workloads.build_constraints(workloads.random_lmi(k=40, r=50, seed=5))
    layer = _layer(cs, wide_kernel="fused64")
    dp = layer.device_pack(DEV)[0]
    assert dp.products_matrix(torch.float64) is not None and lib.rayen_wide_fused64_served(dp.handle) == 0
    x = torch.empty(8, cs.n, 1, dtype=torch.float64).uniform_(-1, 1, generator=torch.Generator().manual_seed(2)).cuda()
    assert _refused(lambda: layer(x)) == _lib.E_UNSUPPORTED
    # a forced 32 beyond its LDS; a tile that does not exist
    dp, v = _pack("s16_first"), _inputs("s16_first", 8)
    assert lib.rayen_wide_fused64_served(dp.handle) == 1
    assert _refused(lambda: ops.project_raw(v, dp, wide_kernel="fused64", wide_samples=32)) == _lib.E_UNSUPPORTED
    assert _refused(lambda: ops.project_raw(v, dp, wide_kernel="fused64", wide_samples=8)) == -1          # RAYEN_E_BAD_ARG
    _run(v, dp)


@pytest.mark.eager_detour
def test_a_refusal_is_announced_once_and_remembered_per_route(monkeypatch):
    monkeypatch.delenv("RAYEN_STRICT_HIP", raising=False)
    cs = F.cs("k129")
    layer = _layer(cs, torch.float32, wide_kernel="fused64")
    x = F.inputs(cs.n, 8).cuda()
    with pytest.warns(RuntimeWarning, match="rayen_amd: no HIP kernel serves"):
        y = layer(x)
    assert layer._refused(x[:, :, 0]) and (0, torch.float32, "fused64") in layer.__dict__["_unsupported"]
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=r"rayen_amd:", category=RuntimeWarning)
        assert torch.equal(layer(x), y)                       # remembered: no second announcement
    want = _layer(cs, torch.float32)(x)
    assert np.max(rel_err_rows(y[:, :, 0].cpu().numpy(), want[:, :, 0].cpu().numpy())) <= FP32_TOL          # fp32 both


# ---------------------------------------------------------------- 6. no effect where it must have none
@pytest.mark.parametrize("which", ["c2", "n64"])
def test_narrow_sets_run_what_they_ran(which):
    """Config 2 (n = 16) and a set with n = 64 do not take the wide route in fp64: the keyword has no effect, bit for bit."""
    cs = workloads.build_constraints(workloads.make_raw("c2", seed=0)) if which == "c2" else C.cs("n64")
    assert cs.n == (16 if which == "c2" else 64)
    x = torch.empty(300, cs.n, 1, dtype=torch.float64).uniform_(-1, 1, generator=torch.Generator().manual_seed(12)).cuda()
    y_default = _layer(cs)(x)
    kernel = _last_kernel()
    y_fused = _layer(cs, wide_kernel="fused64")(x)
    assert _last_kernel() == kernel != _lib.KERNEL_WIDE_FUSED64
    assert torch.equal(y_fused, y_default)
    xg = x.clone().requires_grad_(True)
    assert torch.equal(_layer(cs, wide_kernel="fused64")(xg), y_default)             # the op path


def test_fused_on_fp64_still_refuses():
    cs = C.cs("n65")
    layer = _layer(cs, wide_kernel="fused")
    assert _refused(lambda: layer(_inputs("n65", 8).unsqueeze(2))) == _lib.E_UNSUPPORTED
    assert _lib.load().rayen_wide_fused_served(layer.device_pack(DEV)[0].handle, 1) == 0


# ---------------------------------------------------------------- 7. capture
def test_capture_after_one_call_and_a_fresh_pack_inside_one():
    dp, v = _pack("n65"), _inputs("n65")
    eager = _run(v, dp)                    # the warm call: the image exists from here on
    fresh = DevicePack(C.consts("n65"), 0)
    assert fresh.products_matrix(torch.float64) is not None      # (the route's own upload, in Python: not the kernel's image)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.project_raw(v, dp, wide_kernel="fused64")
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, eager)
    # a pack that has not been asked yet: its first call inside a capture is turned down, nothing is uploaded
    code = []
    other = torch.cuda.CUDAGraph()
    marker = torch.zeros(4, device=DEV)
    with torch.cuda.graph(other):
        marker.add_(1.0)
        try:
            ops.project_raw(v, fresh, wide_kernel="fused64")
        except _lib.RayenError as err:
            code.append(err.code)
    torch.cuda.synchronize()
    assert code == [-8]                    # RAYEN_E_NOT_PREPARED
    assert _same(_run(v, fresh), eager)    # outside the capture it builds its image and serves
