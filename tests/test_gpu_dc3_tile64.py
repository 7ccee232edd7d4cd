"""The fp64 DC3 tile kernels (rayen_amd/csrc/rayen_dc3_tile64.hip) on the MI355X against the fp64 host reference of
tests/dc3_reference.py: every set the fp64 lane kernel refuses and small ones it serves, stop positions around the 32-step
launches, independence from tile-mates, a NaN row, interchange with the fp64 lane kernel, input layouts and graph capture,
the refusals, and ``ConstraintModule`` in fp64 on the corridor set and on a c3-shaped set.

Bar (tests/dc3_tile64_cases.py): ``dc3_cases.row_err`` against the fp64 reference at most 1e-11, ``y`` and ``grad_q``
separately, every row compared; ``steps`` equal to the host's.  tests/test_dc3_tile64_host.py has shown on the host that
every call made here is sound (no residual near a kink at a visited step, the stop decided with 0.5 % to spare)."""
import warnings

import numpy as np
import pytest
import torch

import dc3_cases
import dc3_reference as ref
import dc3_tile64_cases as tc
from rayen_amd import _lib, dc3, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64

_packs = {}


def _pack(key, arrays):
    if key not in _packs:
        _packs[key] = ops.Dc3Pack(arrays, 0)
    return _packs[key]


def _dev(x, dtype=F64):
    return torch.tensor(x).to(dtype).to(DEV)


def _check(label, pack, call, backward=True, fwd="tile64", bwd="tile64"):
    """One forward (+ backward) of ``call`` in fp64 against its host reference, every row.  Returns (y, steps, grad_q)."""
    B, k = call.q.shape[0], pack.k
    q, gy = _dev(call.q), _dev(call.gy)
    y, steps = ops.dc3_forward_raw(q, pack, call.lr, call.momentum, call.eps, call.max_steps, kernel=fwd)
    assert y.shape == (B, k) and y.dtype == F64 and steps.shape == (1,) and steps.dtype == torch.int32
    taken = int(steps.item())
    yh = y.cpu().numpy()
    err_y = dc3_cases.row_err(yh, call.y64).max()
    said = f"{label} B={B} limit={call.max_steps}: steps {taken} (host {call.steps})  y err {err_y:.3e}"
    grad = None
    if backward:
        grad = ops.dc3_backward_raw(q, steps, gy, pack, call.lr, call.momentum, call.max_steps, kernel=bwd)
        assert grad.shape == q.shape and grad.dtype == F64
        gh = grad.cpu().numpy()
        err_g = dc3_cases.row_err(gh, call.gq64).max()
        said += f"  grad err {err_g:.3e}"
    print(said + f"  bar {tc.BAR:.0e}")
    assert taken == call.steps
    assert np.isfinite(yh).all()
    assert err_y <= tc.BAR
    if backward:
        assert np.isfinite(gh).all()
        assert err_g <= tc.BAR
    return y, steps, grad


def _refuses(fn):
    with pytest.raises(_lib.RayenError) as info:
        fn()
    assert info.value.code == _lib.E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 1. every case

@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_every_case_against_the_fp64_reference(case):
    for B, limit, t_star in tc.BACKWARD_CALLS:
        call = tc.call_for(case.name, B, limit, t_star)
        pack = _pack(case.name, call.arrays)
        _, steps, _ = _check(f"{case.name} t*={t_star}", pack, call)
        assert int(steps.item()) == tc.expected_steps(case, limit, t_star)
    for B, limit, t_star in tc.FORWARD_CALLS:
        call = tc.forward_call_for(case.name, B, limit, t_star)
        _, steps, _ = _check(f"{case.name} t*={t_star}", pack, call, backward=False)
        assert int(steps.item()) == tc.expected_steps(case, limit, t_star)
    assert ops.dc3_tile64_served(pack)
    assert ops.dc3_lane_served(pack, F64) == (case in tc.SMALL_CASES)


# ------------------------------------------------------------------------------------------------ 2. stop positions

@pytest.mark.parametrize("position", tc.POSITIONS, ids=lambda p: f"limit{p[0]}-stop{p[1]}")
@pytest.mark.parametrize("name", tc.POSITION_CASES)
def test_stop_positions(name, position):
    max_steps, t_star = position
    call = tc.call_for(name, tc.POSITION_BATCH, max_steps, t_star)
    _, steps, _ = _check(f"{name} t*={t_star}", _pack(name, call.arrays), call)
    assert int(steps.item()) == t_star


# ------------------------------------------------------------------------------------------------ 3. tile-mates

@pytest.mark.parametrize("name", tc.MATES_CASES)
def test_a_row_does_not_depend_on_its_tile_mates_or_on_the_batch(name):
    T = tc.MATES_STEPS
    call = tc.call_for(name, max(tc.MATES_BATCHES), T, None)
    pack = _pack(name, call.arrays)
    q, gy = _dev(call.q), _dev(call.gy)

    def run(B):
        y, steps = ops.dc3_forward_raw(q[:B], pack, call.lr, call.momentum, 0.0, T, kernel="tile64")
        assert int(steps.item()) == T
        return y, ops.dc3_backward_raw(q[:B], steps, gy[:B], pack, call.lr, call.momentum, T, kernel="tile64")

    y_all, g_all = run(max(tc.MATES_BATCHES))
    assert torch.isfinite(y_all).all() and torch.isfinite(g_all).all()
    for B in tc.MATES_BATCHES:
        y, g = run(B)
        assert torch.equal(y, y_all[:B]) and torch.equal(g, g_all[:B]), B
    # a row on its own, from the middle of a tile: the bits do not depend on the column it sits in
    for r in (7, 20):
        y, steps = ops.dc3_forward_raw(q[r:r + 1], pack, call.lr, call.momentum, 0.0, T, kernel="tile64")
        g = ops.dc3_backward_raw(q[r:r + 1], steps, gy[r:r + 1], pack, call.lr, call.momentum, T, kernel="tile64")
        assert torch.equal(y[0], y_all[r]) and torch.equal(g[0], g_all[r]), r


# ------------------------------------------------------------------------------------------------ 4. a NaN row

def test_a_nan_row_keeps_to_itself():
    name = "np8_n5_ragged_everything"
    clean = tc.forward_call_for(name, 33, 40, 7)
    pack = _pack(name, clean.arrays)
    pack.nan_flag.zero_()
    q = _dev(clean.q)
    y_clean, steps = ops.dc3_forward_raw(q, pack, clean.lr, clean.momentum, clean.eps, 40, kernel="tile64")
    assert int(steps.item()) == 7 and int(pack.nan_flag.item()) == 0
    bad = q.clone()
    bad[13, 1] = float("nan")
    y, steps = ops.dc3_forward_raw(bad, pack, clean.lr, clean.momentum, clean.eps, 40, kernel="tile64")
    assert int(steps.item()) == 40                             # NaN < eps is false: the reference runs to the limit
    assert torch.isnan(y[13]).all() and int(pack.nan_flag.item()) == 1
    pack.nan_flag.zero_()
    others = torch.arange(33, device=DEV) != 13
    y0, _ = ops.dc3_forward_raw(q, pack, clean.lr, clean.momentum, 0.0, 40, kernel="tile64")
    y1, _ = ops.dc3_forward_raw(bad, pack, clean.lr, clean.momentum, 0.0, 40, kernel="tile64")
    assert torch.isfinite(y0).all() and torch.equal(y1[others], y0[others]) and torch.isnan(y1[13]).all()
    pack.nan_flag.zero_()


# ------------------------------------------------------------------------------------------------ 5. both kernels of a pack

@pytest.mark.parametrize("case", tc.SMALL_CASES, ids=lambda c: c.name)
def test_interchange_with_the_fp64_lane_kernel(case):
    assert ops.DC3_KERNELS_F64 == ("lane", "tile64")
    for B, limit, t_star in ((65, 10, 7), (33, 40, 33)):
        call = tc.call_for(case.name, B, limit, t_star)
        pack = _pack(case.name, call.arrays)
        for fwd in ops.DC3_KERNELS_F64:
            for bwd in ops.DC3_KERNELS_F64:
                _check(f"{case.name} {fwd} -> {bwd}", pack, call, fwd=fwd, bwd=bwd)


# ------------------------------------------------------------------------------------------------ 6. inputs and capture

def test_layouts_and_the_empty_batch():
    name = "tile_n33_forty_quadratics"
    call = tc.call_for(name, 65, 10, 7)
    pack = _pack(name, call.arrays)
    n, k = pack.n, pack.k
    q, gy = _dev(call.q), _dev(call.gy)

    def run(q, gy):
        y, steps = ops.dc3_forward_raw(q, pack, call.lr, call.momentum, call.eps, 10, kernel="tile64")
        return y, steps, ops.dc3_backward_raw(q, steps, gy, pack, call.lr, call.momentum, 10, kernel="tile64")

    y0, s0, g0 = run(q, gy)
    assert int(s0.item()) == 7 and g0.shape == (65, n)
    wide = torch.full((65, n + 7), float("nan"), device=DEV, dtype=F64)
    wide[:, n + 1:] = 1e300
    wide[:, :n] = q
    yw, sw, gw = run(wide, gy)
    assert torch.equal(yw, y0) and torch.equal(sw, s0) and torch.equal(gw[:, :n], g0) and torch.all(gw[:, n:] == 0)
    strided = wide[:, :n]                                      # row stride n + 7
    assert strided.stride(0) == n + 7
    ys, ss, gs = run(strided, gy)
    assert torch.equal(ys, y0) and torch.equal(ss, s0) and torch.equal(gs, g0)
    gy_wide = torch.full((65, k + 3), float("nan"), device=DEV, dtype=F64)
    gy_wide[:, :k] = gy
    yv, sv, gv = run(q.t().contiguous().t(), gy_wide[:, :k])
    assert torch.equal(yv, y0) and torch.equal(sv, s0) and torch.equal(gv, g0)
    ye, se, ge = run(q[:0], gy[:0])
    assert ye.shape == (0, k) and ge.shape == (0, n) and int(se.item()) == 0


@pytest.mark.parametrize("limit", [10, 40], ids=["one-launch", "two-launches"])
def test_a_captured_forward_and_backward_replays_bit_for_bit(limit):
    name = "tile_n33_forty_quadratics"
    call = tc.call_for(name, 65, 10, 7)
    pack = _pack(name, call.arrays)
    pack_id = ops.register_pack(pack)
    lr, momentum = call.lr, call.momentum
    gy = _dev(call.gy)
    new_q = _dev(ref.make_inputs(tc.CASE[name], 65, seed=1)[0])

    def run(q):
        y, steps = torch.ops.rayen_amd.dc3_project_tile64(q, pack_id, lr, momentum, 0.0, limit)
        (grad,) = torch.autograd.grad(y, q, gy)
        return y, steps, grad

    static_q = _dev(call.q).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static_q)                                          # (warm call: the image is uploaded outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y, static_steps, static_grad = run(static_q)
    with torch.no_grad():
        static_q.copy_(new_q)
    graph.replay()
    torch.cuda.synchronize()
    y, steps, grad = run(new_q.clone().requires_grad_(True))
    assert int(static_steps.item()) == int(steps.item()) == limit
    assert torch.isfinite(y).all() and torch.isfinite(grad).all()
    assert torch.equal(static_y, y) and torch.equal(static_grad, grad)


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_refusals():
    name = "np8_n5_ragged_everything"
    call = tc.call_for(name, 65, 10, 7)
    pack = _pack(name, call.arrays)
    q64, gy64 = _dev(call.q), _dev(call.gy)
    q32, gy32 = q64.float(), gy64.float()
    steps = torch.tensor([3], dtype=torch.int32, device=DEV)
    _refuses(lambda: ops.dc3_forward_raw(q32, pack, call.lr, call.momentum, call.eps, 10, kernel="tile64"))
    _refuses(lambda: ops.dc3_backward_raw(q32, steps, gy32, pack, call.lr, call.momentum, 10, kernel="tile64"))
    _refuses(lambda: ops.dc3_forward_raw(q64, pack, call.lr, call.momentum, call.eps, 10, kernel="tile"))
    _refuses(lambda: ops.dc3_backward_raw(q64, steps, gy64, pack, call.lr, call.momentum, 10, kernel="tile"))
    for kernel in ("wave", "auto", None, "tile32"):
        with pytest.raises(ValueError):
            ops.dc3_forward_raw(q64, pack, call.lr, call.momentum, call.eps, 10, kernel=kernel)
        with pytest.raises(ValueError):
            ops.dc3_backward_raw(q64, steps, gy64, pack, call.lr, call.momentum, 10, kernel=kernel)
    beyond = ref.Case("n65_beyond_the_registers", 65, 1, 0, 0, 1e-2, 0.5)
    pack65 = _pack(beyond.name, ref.make_pack(beyond))
    q, gy = (_dev(x) for x in ref.make_inputs(beyond, 33))
    for kernel in ops.DC3_KERNELS_F64:
        _refuses(lambda: ops.dc3_forward_raw(q, pack65, beyond.lr, ref.MOMENTUM, 1e-3, 10, kernel=kernel))
        _refuses(lambda: ops.dc3_backward_raw(q, steps, gy, pack65, beyond.lr, ref.MOMENTUM, 10, kernel=kernel))
    for kernel in ops.DC3_KERNELS + ("tile64",):               # (and every kernel refuses it in fp32)
        _refuses(lambda: ops.dc3_forward_raw(q.float(), pack65, beyond.lr, ref.MOMENTUM, 1e-3, 10, kernel=kernel))
    assert not ops.dc3_tile64_served(pack65) and not ops.dc3_lane_served(pack65, F64)


def test_a_pack_allocates_an_image_only_when_asked():
    case = tc.CASE["np32_n17_one_quadratic"]
    pack = ops.Dc3Pack(ref.make_pack(case), 0)
    served = _lib.load().rayen_dc3_tile64_served
    q = _dev(ref.make_inputs(case, 5)[0])
    ops.dc3_forward_raw(q, pack, case.lr, ref.MOMENTUM, 0.0, 3)                   # the lane kernel
    ops.dc3_forward_raw(q.float(), pack, case.lr, ref.MOMENTUM, 0.0, 3, kernel="tile")
    assert served(pack.handle) == 0 and pack._arrays is not None                  # the fp32 upload was not the last
    ops.dc3_forward_raw(q, pack, case.lr, ref.MOMENTUM, 0.0, 3, kernel="tile64")
    assert served(pack.handle) == 1 and pack._arrays is None
    pack.close()


# ------------------------------------------------------------------------------------------------ 8. the module in fp64

C5_ARGS = dict(lr=1e-5, momentum=0.5, eps_converge=0.0, max_steps_training=7, max_steps_testing=40)     # test_gpu_dc3_tile.py's
C3_ARGS = dict(lr=2e-5, momentum=0.5, eps_converge=0.0, max_steps_training=7, max_steps_testing=40)


def _constraints(which):
    if which == "c5":
        return workloads.build_constraints(workloads.make_raw("c5")), C5_ARGS
    raw = workloads.random_lin_quad_soc(k=64, m=128, n_quad=4, n_soc=0, seed=2)       # config 3's shape, its cones dropped
    return workloads.build_constraints(raw), C3_ARGS


def _layer(which, kernel):
    cs, args = _constraints(which)
    args = dict(args) if kernel is None else dict(args, kernel=kernel)
    return ConstraintModule(cs, method="DC3", args_DC3=args, create_map=False)


@pytest.mark.parametrize("kernel", ["tile", "auto"])
@pytest.mark.parametrize("which", ["c5", "c3"])
def test_module_in_fp64(which, kernel, monkeypatch):
    monkeypatch.setenv("RAYEN_STRICT_HIP", "1")
    host = _layer(which, kernel)
    layer = _layer(which, kernel).to(DEV)
    args = C5_ARGS if which == "c5" else C3_ARGS
    arrays = dc3.pack_arrays(host)
    n = int(arrays["n"])
    shape = (n, arrays["A1e"].shape[0], arrays["Pe"].shape[0], arrays["k"] - n)
    assert shape == ((30, 1050, 72, 15) if which == "c5" else (64, 128, 4, 0))
    assert layer.dc3_kernel == kernel
    monkeypatch.setattr(layer, "_dc3_reference", lambda *a, **k: (_ for _ in ()).throw(AssertionError("eager detour")))
    q = (0.25 * torch.randn(33, n, 1, generator=torch.Generator().manual_seed(17))).double()
    for training, limit in ((True, 7), (False, 40)):
        host.train(training)
        layer.train(training)
        with torch.no_grad():
            y64 = dc3.reference_forward(host, q)[:, :, 0].numpy()
        assert np.isfinite(y64).all()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            y = layer(q.to(DEV))
        assert y.dtype == F64 and layer.dc3_steps.tolist() == [limit] and not layer._hip_unsupported
        err = dc3_cases.row_err(y.cpu()[:, :, 0].numpy(), y64).max()
        print(f"{which} {kernel} fp64 limit {limit}: y err {err:.3e} bar {tc.BAR:.0e}")
        assert err <= tc.BAR
    # the gradient of (y * g).sum() after the 7 training steps, against autograd through the fp64 formula, every row
    host.train(True)
    layer.train(True)
    g = torch.randn(33, host.k, 1, generator=torch.Generator().manual_seed(18)).double()
    qh = q.clone().requires_grad_(True)
    (dc3.reference_forward(host, qh) * g).sum().backward()
    want = qh.grad[:, :, 0].numpy()
    res = ref.forward_ref(arrays, q[:, :, 0].numpy(), args["lr"], 0.5, 0.0, 7).res
    assert tc.nearest_residual(res) > tc.KINK_REL              # (the condition on the inputs under which every row counts)
    qd = q.to(DEV).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        (layer(qd) * g.to(DEV)).sum().backward()
    got = qd.grad.cpu()[:, :, 0].numpy()
    assert np.isfinite(got).all()
    err = dc3_cases.row_err(got, want).max()
    print(f"{which} {kernel} fp64 grad err {err:.3e} bar {tc.BAR:.0e}  nearest residual {tc.nearest_residual(res):.2e}")
    assert err <= tc.BAR
    assert not layer._hip_unsupported
    dp, _ = layer.dc3_pack(torch.device(DEV))
    assert layer._dc3_kernel_for(dp, F64) == "tile64" and not ops.dc3_lane_served(dp, F64)


@pytest.mark.parametrize("which", ["c5", "c3"])
def test_the_default_kernel_still_refuses_in_fp64(which, monkeypatch):
    monkeypatch.setenv("RAYEN_STRICT_HIP", "1")
    for kernel in (None, "lane"):
        plain = _layer(which, kernel).to(DEV)
        assert plain.dc3_kernel == "lane"
        q = (0.25 * torch.randn(33, plain.dim_after_map, 1, generator=torch.Generator().manual_seed(17))).double().to(DEV)
        with pytest.raises(_lib.RayenError) as info:
            plain(q)
        assert info.value.code == _lib.E_UNSUPPORTED
