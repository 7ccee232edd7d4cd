"""The DC3 tile kernels (rayen_amd/csrc/rayen_dc3_tile.hip) on the MI355X against the fp64 host reference of
tests/dc3_reference.py: four sets beyond the lane kernel's LDS image, every fp32 case and stop position of the lane kernel's
sweep through ``kernel='tile'``, the deciding row in the last partial tile, independence from tile-mates, interchange with
the lane kernel, a NaN row, input layouts and graph capture, the refusals, and ``ConstraintModule`` on the corridor set.

Bars (those of tests/test_gpu_dc3_sweep.py): ``dc3_cases.row_err`` against the fp64 reference at most max(4 x the host's own
fp32-versus-fp64 gap of the same call and rows, 1e-5), ``y`` and ``grad_q`` separately; ``steps`` equal to the host's.  The
backward is compared outside the rows of ``dc3_tile_cases.wide_kink_rows``, whose number is capped (a condition on the
inputs that tests/test_dc3_tile_host.py has shown on the host)."""
import warnings

import numpy as np
import pytest
import torch

import dc3_cases
import dc3_reference as ref
import dc3_tile_cases as tc
from rayen_amd import _lib, dc3, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-5
F32 = torch.float32

_packs = {}


def _pack(key, arrays):
    if key not in _packs:
        _packs[key] = ops.Dc3Pack(arrays, 0)
    return _packs[key]


def _dev(x, dtype=F32):
    return torch.tensor(x).to(dtype).to(DEV)


def _bars(call, rows, keep):
    gap_y, gap_g = ref.gaps(call, rows, keep)
    return max(4.0 * gap_y, FLOOR), max(4.0 * gap_g, FLOOR)


def _check(label, pack, call, rows=None, backward=True, fwd="tile", bwd="tile"):
    """One forward (+ backward) of ``call`` in fp32 against its host reference (``rows``: the rows compared, all by
    default).  Returns (y, steps, grad_q) as the kernels left them."""
    B, n, k = call.q.shape[0], pack.n, pack.k
    rows = np.ones(B, dtype=bool) if rows is None else rows
    q, gy = _dev(call.q), _dev(call.gy)
    y, steps = ops.dc3_forward_raw(q, pack, call.lr, call.momentum, call.eps, call.max_steps, kernel=fwd)
    assert y.shape == (B, k) and y.dtype == F32 and steps.shape == (1,) and steps.dtype == torch.int32
    taken = int(steps.item())
    yh = y.cpu().numpy()
    keep = rows & ~call.kinks
    bar_y, bar_g = _bars(call, rows, keep)
    err_y = dc3_cases.row_err(yh[rows], call.y64[rows]).max()
    said = f"{label} B={B} limit={call.max_steps}: steps {taken} (host {call.steps})  y err {err_y:.3e} bar {bar_y:.3e}"
    grad = None
    if backward:
        grad = ops.dc3_backward_raw(q, steps, gy, pack, call.lr, call.momentum, call.max_steps, kernel=bwd)
        assert grad.shape == q.shape and grad.dtype == F32
        gh = grad.cpu().numpy()
        err_g = dc3_cases.row_err(gh[keep], call.gq64[keep]).max() if keep.any() else 0.0
        said += f"  grad err {err_g:.3e} bar {bar_g:.3e}  kinks {int(call.kinks.sum())}"
    print(said)
    assert taken == call.steps
    assert np.isfinite(yh[rows]).all()
    assert err_y <= bar_y
    if backward:
        assert np.isfinite(gh[rows]).all()
        assert int(call.kinks[rows].sum()) <= ref.kink_cap(B)
        assert err_g <= bar_g
    return y, steps, grad


def _lane_refuses(pack, call, backward):
    q, gy = _dev(call.q), _dev(call.gy)
    with pytest.raises(_lib.RayenError) as info:
        ops.dc3_forward_raw(q, pack, call.lr, call.momentum, call.eps, call.max_steps)
    assert info.value.code == _lib.E_UNSUPPORTED
    if backward:
        steps = torch.tensor([call.steps], dtype=torch.int32, device=DEV)
        with pytest.raises(_lib.RayenError) as info:
            ops.dc3_backward_raw(q, steps, gy, pack, call.lr, call.momentum, call.max_steps)
        assert info.value.code == _lib.E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 1. beyond the lane kernel

@pytest.mark.parametrize("case", tc.TILE_CASES, ids=lambda c: c.name)
def test_sets_beyond_the_lane_kernels_image(case):
    assert not ref.served(case, F32)
    for B, limit, t_star in tc.BACKWARD_CALLS:
        call = tc.call_for(case.name, B, limit, t_star)
        pack = _pack(case.name, call.arrays)
        _lane_refuses(pack, call, True)
        _check(f"{case.name} t*={t_star}", pack, call)
    for B, limit, t_star in tc.FORWARD_CALLS:
        call = tc.forward_call_for(case.name, B, limit, t_star)
        pack = _pack(case.name, call.arrays)
        _lane_refuses(pack, call, False)
        _, steps, _ = _check(f"{case.name} t*={t_star}", pack, call, backward=False)
        assert int(steps.item()) == (limit if t_star is None else t_star)
    assert ops.dc3_tile_served(pack) and not ops.dc3_lane_served(pack, F32)


# ------------------------------------------------------------------------------------------------ 2. the lane kernel's sweep

@pytest.mark.parametrize("case", tc.sweep_cases(), ids=lambda c: c.name)
def test_every_case_of_the_lane_sweep(case):
    for B in ref.SWEEP_BATCHES:
        for position in (ref.TRAIN_CALL, ref.EVAL_CALL):
            call = tc.call_for(case.name, B, *position)
            pack = _pack(case.name, call.arrays)
            _check(f"{case.name} t*={position[1]}", pack, call)
    assert ops.dc3_tile_served(pack) and ops.dc3_lane_served(pack, F32)


# ------------------------------------------------------------------------------------------------ 3. stop positions

@pytest.mark.parametrize("position", ref.POSITIONS, ids=lambda p: f"limit{p[0]}-stop{p[1]}")
@pytest.mark.parametrize("name", ref.POSITION_CASES)
def test_stop_positions(name, position):
    max_steps, t_star = position
    call = tc.call_for(name, ref.POSITION_BATCH, max_steps, t_star)
    _, steps, _ = _check(f"{name} t*={t_star}", _pack(name, call.arrays), call)
    assert int(steps.item()) == (max_steps if t_star is None else t_star)


# ------------------------------------------------------------------------------------------------ 4. the last, partial tile

@pytest.mark.parametrize("B", tc.OUTLIER_BATCHES)
def test_deciding_row_in_the_last_partial_tile(B):
    far, near = tc.outlier_calls(B)
    pack = _pack("outlier", far.arrays)
    _, steps_far, _ = _check(f"outlier row {B - 1}", pack, far)
    _, steps_near, _ = _check("outlier row replaced", pack, near)
    # the pad columns of the last tile sit at the origin, outside this set: they must not hold the stop back
    assert int(steps_near.item()) == near.steps == 1 < int(steps_far.item()) == ref.OUTLIER_CALL[1]


# ------------------------------------------------------------------------------------------------ 5. tile-mates

@pytest.mark.parametrize("name", tc.MATES_CASES)
def test_a_column_does_not_depend_on_its_tile_mates(name):
    call = tc.call_for(name, 257, 10, None)
    pack = _pack(name, call.arrays)
    q, gy = _dev(call.q), _dev(call.gy)

    def run(B):
        y, steps = ops.dc3_forward_raw(q[:B], pack, call.lr, call.momentum, 0.0, 10, kernel="tile")
        assert int(steps.item()) == 10
        return y, ops.dc3_backward_raw(q[:B], steps, gy[:B], pack, call.lr, call.momentum, 10, kernel="tile")

    y_all, g_all = run(257)
    assert torch.isfinite(y_all).all() and torch.isfinite(g_all).all()
    for B in tc.MATES_BATCHES:
        y, g = run(B)
        assert torch.equal(y, y_all[:B]) and torch.equal(g, g_all[:B]), B


# ------------------------------------------------------------------------------------------------ 6. interchange

def test_interchange_with_the_lane_kernel():
    name = "np32_n32_full"
    for position in (ref.TRAIN_CALL, ref.EVAL_CALL):
        call = tc.call_for(name, 65, *position)
        pack = _pack(name, call.arrays)
        ys = {}
        for fwd in ops.DC3_KERNELS:
            for bwd in ops.DC3_KERNELS:
                ys[fwd], _, _ = _check(f"{name} {fwd} -> {bwd}", pack, call, fwd=fwd, bwd=bwd)
        bar_y, _ = _bars(call, np.ones(65, dtype=bool), ~call.kinks)
        assert dc3_cases.row_err(ys["tile"].cpu().numpy(), ys["lane"].cpu().numpy()).max() <= 2.0 * bar_y


# ------------------------------------------------------------------------------------------------ 7. a NaN row

def test_a_nan_row_keeps_to_itself():
    name = "np8_n5_ragged_everything"
    clean = tc.forward_call_for(name, 33, 40, 7)
    pack = _pack(name, clean.arrays)
    pack.nan_flag.zero_()
    q = _dev(clean.q)
    y_clean, steps = ops.dc3_forward_raw(q, pack, clean.lr, clean.momentum, clean.eps, 40, kernel="tile")
    assert int(steps.item()) == 7 and int(pack.nan_flag.item()) == 0
    bad = q.clone()
    bad[13, 1] = float("nan")
    y, steps = ops.dc3_forward_raw(bad, pack, clean.lr, clean.momentum, clean.eps, 40, kernel="tile")
    assert int(steps.item()) == 40                             # NaN < eps is false: the reference runs to the limit
    assert torch.isnan(y[13]).all() and int(pack.nan_flag.item()) == 1
    pack.nan_flag.zero_()
    others = torch.arange(33, device=DEV) != 13
    y0, _ = ops.dc3_forward_raw(q, pack, clean.lr, clean.momentum, 0.0, 40, kernel="tile")
    y1, _ = ops.dc3_forward_raw(bad, pack, clean.lr, clean.momentum, 0.0, 40, kernel="tile")
    assert torch.isfinite(y0).all() and torch.equal(y1[others], y0[others]) and torch.isnan(y1[13]).all()
    pack.nan_flag.zero_()


# ------------------------------------------------------------------------------------------------ 8. inputs and capture

def test_layouts_and_the_empty_batch():
    name = "tile_n33_forty_quadratics"
    call = tc.call_for(name, 65, 10, 7)
    pack = _pack(name, call.arrays)
    n, k = pack.n, pack.k
    q, gy = _dev(call.q), _dev(call.gy)

    def run(q, gy):
        y, steps = ops.dc3_forward_raw(q, pack, call.lr, call.momentum, call.eps, 10, kernel="tile")
        return y, steps, ops.dc3_backward_raw(q, steps, gy, pack, call.lr, call.momentum, 10, kernel="tile")

    y0, s0, g0 = run(q, gy)
    assert int(s0.item()) == 7 and g0.shape == (65, n)
    wide = torch.full((65, n + 7), float("nan"), device=DEV)
    wide[:, n + 1:] = 1e30
    wide[:, :n] = q
    yw, sw, gw = run(wide, gy)
    assert torch.equal(yw, y0) and torch.equal(sw, s0) and torch.equal(gw[:, :n], g0) and torch.all(gw[:, n:] == 0)
    gy_wide = torch.full((65, k + 3), float("nan"), device=DEV)
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
    new_q = _dev(ref.make_inputs(tc.TILE_CASE[name], 65, seed=1)[0])

    def run(q):
        y, steps = torch.ops.rayen_amd.dc3_project_tile(q, pack_id, lr, momentum, 0.0, limit)
        (grad,) = torch.autograd.grad(y, q, gy)
        return y, steps, grad

    static_q = _dev(call.q).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static_q)                                          # (warm-up: the tile image is uploaded outside the capture)
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


# ------------------------------------------------------------------------------------------------ 9. refusals

def test_refusals():
    name = "np8_n5_ragged_everything"
    call = tc.call_for(name, 65, *ref.TRAIN_CALL)
    pack = _pack(name, call.arrays)
    q64, gy64 = _dev(call.q, torch.float64), _dev(call.gy, torch.float64)
    steps = torch.tensor([3], dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.RayenError) as info:
        ops.dc3_forward_raw(q64, pack, call.lr, call.momentum, call.eps, 10, kernel="tile")
    assert info.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(_lib.RayenError) as info:
        ops.dc3_backward_raw(q64, steps, gy64, pack, call.lr, call.momentum, 10, kernel="tile")
    assert info.value.code == _lib.E_UNSUPPORTED
    for kernel in ("wave", "auto", None):
        with pytest.raises(ValueError):
            ops.dc3_forward_raw(q64.float(), pack, call.lr, call.momentum, call.eps, 10, kernel=kernel)
        with pytest.raises(ValueError):
            ops.dc3_backward_raw(q64.float(), steps, gy64.float(), pack, call.lr, call.momentum, 10, kernel=kernel)
    beyond = ref.Case("n65_beyond_the_registers", 65, 1, 0, 0, 1e-2, 0.5)
    pack65 = _pack(beyond.name, ref.make_pack(beyond))
    q, gy = (_dev(x) for x in ref.make_inputs(beyond, 33))
    for kernel in ops.DC3_KERNELS:
        with pytest.raises(_lib.RayenError) as info:
            ops.dc3_forward_raw(q, pack65, beyond.lr, ref.MOMENTUM, 1e-3, 10, kernel=kernel)
        assert info.value.code == _lib.E_UNSUPPORTED
        with pytest.raises(_lib.RayenError) as info:
            ops.dc3_backward_raw(q, steps, gy, pack65, beyond.lr, ref.MOMENTUM, 10, kernel=kernel)
        assert info.value.code == _lib.E_UNSUPPORTED
    assert not ops.dc3_tile_served(pack65) and not ops.dc3_lane_served(pack65, F32)


# ------------------------------------------------------------------------------------------------ 10. the corridor set

C5_ARGS = dict(lr=1e-5, momentum=0.5, eps_converge=0.0, max_steps_training=7, max_steps_testing=40)


def _c5_layer(kernel=None, **kw):
    args = dict(C5_ARGS) if kernel is None else dict(C5_ARGS, kernel=kernel)
    cs = workloads.build_constraints(workloads.make_raw("c5"))
    return ConstraintModule(cs, method="DC3", args_DC3=args, **kw)


def _c5_input(B=33):
    return 0.25 * torch.randn(B, 30, 1, generator=torch.Generator().manual_seed(17))


@pytest.mark.parametrize("kernel", ["tile", "auto"])
def test_module_on_the_corridor_set(kernel, monkeypatch):
    monkeypatch.setenv("RAYEN_STRICT_HIP", "1")
    host = _c5_layer(kernel, create_map=False)
    layer = _c5_layer(kernel, create_map=False).to(DEV)
    assert layer.dc3_kernel == kernel and layer.dim_after_map == 30
    arrays = dc3.pack_arrays(host)
    assert (arrays["n"], arrays["A1e"].shape[0], arrays["Pe"].shape[0], arrays["k"] - arrays["n"]) == tc.CORRIDOR_SHAPE
    monkeypatch.setattr(layer, "_dc3_reference", lambda *a, **k: (_ for _ in ()).throw(AssertionError("eager detour")))
    q = _c5_input()
    for training, limit in ((True, 7), (False, 40)):
        host.train(training)
        layer.train(training)
        with torch.no_grad():
            y64 = dc3.reference_forward(host, q.double())[:, :, 0].numpy()
            y32 = dc3.reference_forward(host, q)[:, :, 0].numpy()
        assert np.isfinite(y64).all() and np.isfinite(y32).all()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            y = layer(q.to(DEV))
        assert layer.dc3_steps.tolist() == [limit] and not layer._hip_unsupported
        bar = max(4.0 * dc3_cases.row_err(y32, y64).max(), FLOOR)
        err = dc3_cases.row_err(y.cpu()[:, :, 0].numpy(), y64).max()
        print(f"c5 {kernel} limit {limit}: y err {err:.3e} bar {bar:.3e}")
        assert err <= bar
    # the gradient of (y * g).sum() after the 7 training steps, against autograd through the fp64 formula
    host.train(True)
    layer.train(True)
    g = torch.randn(33, host.k, 1, generator=torch.Generator().manual_seed(18))
    grads = {}
    for dt in (torch.float64, torch.float32):
        qh = q.to(dt).clone().requires_grad_(True)
        (dc3.reference_forward(host, qh) * g.to(dt)).sum().backward()
        grads[dt] = qh.grad[:, :, 0].double().numpy()
    res = {dt: ref.forward_ref(arrays, q[:, :, 0].numpy(), C5_ARGS["lr"], 0.5, 0.0, 7, dt).res[:-1]
           for dt in (torch.float64, torch.float32)}          # the residuals at p_0 .. p_6: where the backward looks
    kinks = tc.wide_kink_rows(res[torch.float64], res[torch.float32])
    assert int(kinks.sum()) <= ref.kink_cap(33)
    qd = q.to(DEV).requires_grad_(True)
    (layer(qd) * g.to(DEV)).sum().backward()
    got = qd.grad.cpu()[:, :, 0].numpy()
    assert np.isfinite(got).all()
    bar = max(4.0 * dc3_cases.row_err(grads[torch.float32][~kinks], grads[torch.float64][~kinks]).max(), FLOOR)
    err = dc3_cases.row_err(got[~kinks], grads[torch.float64][~kinks]).max()
    print(f"c5 {kernel} grad err {err:.3e} bar {bar:.3e} kinks {int(kinks.sum())}")
    assert err <= bar
    assert not layer._hip_unsupported


def test_module_on_the_corridor_set_default_nan_and_training(monkeypatch):
    q = _c5_input().to(DEV)
    plain = _c5_layer(None, create_map=False).to(DEV)
    assert plain.dc3_kernel == "lane"
    monkeypatch.setenv("RAYEN_STRICT_HIP", "1")
    with pytest.raises(_lib.RayenError):
        plain(q)                                               # the default kernel still refuses this set
    layer = _c5_layer("tile", create_map=False).to(DEV).eval()
    bad = q.clone()
    bad[7, 1, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"args_DC3\['lr'\]"):
        layer(bad)
    layer(q)                                                   # the flag was cleared
    # five SGD steps through a mapper lower a squared-distance loss
    torch.manual_seed(5)                                        # (the mapper's weights)
    net = _c5_layer("tile", input_dim=7).to(DEV).train()
    monkeypatch.setattr(net, "_dc3_reference", lambda *a, **k: (_ for _ in ()).throw(AssertionError("eager detour")))
    x = (0.25 * torch.randn(33, 7, 1, generator=torch.Generator().manual_seed(31))).to(DEV)
    with torch.no_grad():
        target = net(x).detach() * 0.5
    opt = torch.optim.SGD(net.mapper.parameters(), lr=1e-2)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = (net(x) - target).square().sum(dim=1).mean()
        loss.backward()
        assert torch.isfinite(net.mapper.weight.grad).all()
        losses.append(float(loss.detach()))
        opt.step()
    print("c5 mapper losses", losses)
    assert losses[-1] < losses[0] and not net._hip_unsupported
