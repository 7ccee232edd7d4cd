"""The streamed soft-cost kernels (rayen_amd/csrc/rayen_cost_stream.hip: the image of the stacked rows through LDS in
windows) through ``ops.soft_cost_raw(kernel='stream')``, ``rayen_amd::soft_cost_stream``, the raw C ABI and the module.

1  Where the resident kernels (rayen_cost.hip) serve a set, the streamed result is theirs bit for bit -- ``torch.equal`` on
   cost, worst, which and grad, at the smallest legal window, at three tiles' worth and at the default.
2  Beyond the resident envelope the results are held to the fp64 reference by ``helpers.cost_check`` at the bars of
   tests/cost_reference.py, unchanged: the arithmetic and the chain depths are the resident kernels'.
The cases are tests/cost_stream_cases.py; tests/test_cost_stream_host.py checks the window partition on the host."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cost_cases                                             # noqa: E402
import cost_lmi_cases as L                                    # noqa: E402
import cost_stream_cases as S                                 # noqa: E402
import cost_sweep_cases as sweep                              # noqa: E402
from helpers import cost_check as _check                      # noqa: E402
from helpers import cost_device_y as _device_y                # noqa: E402
from rayen_amd import _lib, ops, soft_cost                    # noqa: E402
from rayen_amd.cost_computer import CostComputer              # noqa: E402
from rayen_amd.soft_cost import SoftCost                      # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ["float32", "float64"]
CANARY = 12345.0
_PACKS = {}


def _pack(arrays):
    key = id(arrays)
    if key not in _PACKS:
        _PACKS[key] = (arrays, ops.CostPack(arrays, torch.cuda.current_device()))
    return _PACKS[key][1]


def _same(a, b):
    """Bit for bit, NaNs included."""
    if a.dtype.is_floating_point:
        ints = torch.int32 if a.dtype == torch.float32 else torch.int64
        return torch.equal(a.contiguous().view(ints), b.contiguous().view(ints))
    return torch.equal(a, b)


def _all_same(got, want):
    return all(_same(a, b) for a, b in zip(got, want))


def _abi(pack, dtype_name, y, B, ld, cost, worst, which, grad, ldg, stream=True):
    lib = _lib.load()
    fn = getattr(lib, ("rayen_soft_cost_stream_" if stream else "rayen_soft_cost_") + ("f32" if dtype_name == "float32" else "f64"))
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    code = fn(pack.handle, ptr(y), B, ld, ptr(cost), ptr(worst), ptr(which), ptr(grad), ldg,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code


def _laid_out(dtype, B, k, kind, fill):
    off, ld = sweep.layout(kind, k)
    lead = (ld + 3) // 4 * 4
    flat = torch.full((lead + off + B * ld + 8,), fill, dtype=dtype, device="cuda")
    rows = flat.as_strided((B, k), (ld, 1), lead + off)
    assert (rows.data_ptr() % 16 == 0) == (off == 0) and rows.stride(0) == ld
    return flat, rows


# ---- 1 bit-equality with the resident kernels

@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("name", list(S.SHARED))
def test_streamed_is_the_resident_result_bit_for_bit(name, dtype_name):
    c = S.SHARED[name]()
    dtype, pack = getattr(torch, dtype_name), _pack(c.arrays)
    if not pack.served(dtype):
        assert (name, dtype_name) in S.SHARED_REFUSED
        return
    assert (name, dtype_name) not in S.SHARED_REFUSED
    y = _device_y(c, dtype_name)
    want = ops.soft_cost_raw(y, pack, True)
    for window in S.forced_windows(c.arrays, dtype_name):
        what = f"{name} {dtype_name} window {window}"
        assert pack.stream_served(dtype, window), what
        got = ops.soft_cost_raw(y, pack, True, kernel="stream")
        assert _all_same(got, want), what
        # values alone (grad = NULL: the other kernel variant), and a second call repeats the first
        cost0, worst0, which0, none = ops.soft_cost_raw(y, pack, False, kernel="stream")
        assert none is None and _all_same((cost0, worst0, which0), want), what
        assert _all_same(ops.soft_cost_raw(y, pack, True, kernel="stream"), want), what
    # the resident route answers as before, whatever was streamed
    assert _all_same(ops.soft_cost_raw(y, pack, True), want)


@pytest.mark.parametrize("name,dtype_name", [("tile_mixed", "float32"), ("tile_mixed", "float64")])
def test_layouts_bit_for_bit(name, dtype_name):
    """Offset bases and a row stride of k + 1 for y and for grad, independently: the scalar paths of the loads and stores."""
    c = S.SHARED[name]()
    dtype, pack, k = getattr(torch, dtype_name), _pack(c.arrays), c.arrays["k"]
    B = c.y.shape[0]
    data = torch.from_numpy(c.y.copy()).to(dtype).cuda()
    want = ops.soft_cost_raw(data, pack, True)
    assert pack.stream_served(dtype, S.forced_windows(c.arrays, dtype_name)[1])
    for y_kind in sweep.LAYOUTS:
        for g_kind in sweep.LAYOUTS:
            what = f"{name} {dtype_name} y {y_kind} grad {g_kind}"
            _, y = _laid_out(dtype, B, k, y_kind, float("nan"))
            y.copy_(data)
            gflat, grad = _laid_out(dtype, B, k, g_kind, CANARY)
            cost = torch.full((B + 2,), CANARY, dtype=dtype, device="cuda")
            worst, which = cost.clone(), torch.full((B + 2,), 777, dtype=torch.int32, device="cuda")
            assert _abi(pack, dtype_name, y, B, y.stride(0), cost[1:], worst[1:], which[1:], grad, grad.stride(0)) == 0, what
            assert _all_same((cost[1:B + 1], worst[1:B + 1], which[1:B + 1], grad), want), what
            assert float(cost[0]) == CANARY == float(cost[B + 1]) and float(worst[0]) == CANARY == float(worst[B + 1]), what
            assert int(which[0]) == 777 == int(which[B + 1]), what
            grad.fill_(CANARY)
            assert bool((gflat == CANARY).all()), what


# ---- 2 beyond the resident envelope, against the fp64 reference

@pytest.mark.parametrize("name,dtype_name", S.BEYOND_PARAMS)
def test_beyond_the_resident_envelope_against_the_reference(name, dtype_name):
    c = S.beyond_case(name)
    dtype, pack = getattr(torch, dtype_name), _pack(c.arrays)
    assert not pack.served(dtype)
    with pytest.raises(_lib.RayenError) as err:          # the resident route refuses as before
        ops.soft_cost_raw(_device_y(c, dtype_name), pack, True)
    assert err.value.code == _lib.E_UNSUPPORTED
    y = _device_y(c, dtype_name).requires_grad_(True)
    first = None
    for window in reversed(S.forced_windows(c.arrays, dtype_name)):          # the default first
        what = f"{name} {dtype_name} window {window} stream"
        assert pack.stream_served(dtype, window), what
        if first is None:
            pack_id = ops.register_pack(pack)
            cost, worst, which, grad = torch.ops.rayen_amd.soft_cost_stream(y, pack_id, True)
            _check(c, dtype_name, cost.detach(), worst, which, grad, what)
            go = torch.from_numpy(np.random.default_rng(5).uniform(0.5, 2.0, size=cost.shape[0])).to(cost.dtype).cuda()
            (gy,) = torch.autograd.grad(cost, y, go)
            assert _same(gy, go[:, None] * grad), what
            first = (cost.detach(), worst, which, grad)
            cost0, worst0, which0, none = ops.soft_cost_raw(y.detach(), pack, False, kernel="stream")
            assert none is None and _all_same((cost0, worst0, which0), first), what
        else:          # the window size moves the cuts, not a bit of the result
            assert _all_same(ops.soft_cost_raw(y.detach(), pack, True, kernel="stream"), first), what


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("B", S.CORRIDOR_BATCHES)
def test_batches(B, dtype_name):
    """1, 31, 129 and 257 rows: a partial group, a workgroup whose last waves (fp32: at 129, three of the second workgroup's
    four) have no live sample and still take every barrier, lanes beyond B in fp64."""
    c = S.corridor_case(B)
    dtype, pack = getattr(torch, dtype_name), _pack(S.corridor_set())
    assert pack.stream_served(dtype, S.forced_windows(c.arrays, dtype_name)[1])
    y = _device_y(c, dtype_name)
    cost = torch.full((B + 2,), CANARY, dtype=dtype, device="cuda")
    worst, which = cost.clone(), torch.full((B + 2,), 777, dtype=torch.int32, device="cuda")
    grad = torch.full((B + 2, c.arrays["k"]), CANARY, dtype=dtype, device="cuda")
    assert _abi(pack, dtype_name, y, B, y.stride(0), cost[1:], worst[1:], which[1:], grad[1:], grad.stride(0)) == 0
    _check(c, dtype_name, cost[1:B + 1], worst[1:B + 1], which[1:B + 1], grad[1:B + 1], f"{c.name} {dtype_name} stream")
    for t in (cost, worst, grad):
        assert bool((t[0] == CANARY).all()) and bool((t[B + 1] == CANARY).all())
    assert int(which[0]) == 777 == int(which[B + 1])
    # the first rows of the larger batch are these rows: samples do not mix
    if B < 257:
        big = ops.soft_cost_raw(_device_y(S.corridor_case(), dtype_name), pack, True, kernel="stream")
        assert _all_same((cost[1:B + 1], worst[1:B + 1], which[1:B + 1], grad[1:B + 1]), tuple(t[:B] for t in big))


# ---- 2b more than one pass of a workgroup over the sample groups (every production batch)

def _passes_batch(dtype_name):
    """Rows that give every workgroup of the persistent grid at least three passes (four rounds are dealt): fp32 groups of
    32 rows over four waves per CU, fp64 blocks of 256 rows over the CUs; a partial last group."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return 3 * 128 * cus + 33 if dtype_name == "float32" else 3 * 256 * cus + 257


def _parity_windows(a, dtype_name):
    """(window, nw) with an odd and with an even number of windows, both > 1, and the default: from the second pass on the
    buffer of window 0 alternates when nw is odd and stays when it is even."""
    K = sweep.lane64_K(a["k"])
    its = S.items(a, dtype_name)
    small = S.smallest_window(a, dtype_name)
    step = S.TILE_BYTES32 if dtype_name == "float32" else (8 * (K + 1) * 8 + 15) // 16 * 16
    found = {}
    for j in range(400):
        window = small + j * step
        if window > S.DEFAULT_WINDOW:
            break
        nw = len(S.partition(its, dtype_name, K, window))
        if nw > 1:
            found.setdefault(nw % 2, (window, nw))
    assert set(found) == {0, 1}, found
    return [found[1], found[0], (0, len(S.partition(its, dtype_name, K, S.DEFAULT_WINDOW)))]


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("name", ["tile_mixed", "corridor_k12"])
def test_several_passes_per_workgroup(name, dtype_name):
    """The prefetch of window 0 for the next sample groups under the last window's walk, the buffer parity from the second
    pass on, and y loads / stores issued while a copy is in flight: a batch of three and more passes per workgroup, the rows
    of the small case repeated.  ``tile_mixed`` (both routes serve it): the resident kernel's bits on the same batch.
    ``corridor_k12`` (beyond the resident envelope): the streamed result of the 257 rows, repeated -- samples do not mix."""
    c = S.SHARED[name]() if name in S.SHARED else S.beyond_case(name)
    dtype, pack = getattr(torch, dtype_name), _pack(c.arrays)
    B, n = _passes_batch(dtype_name), c.y.shape[0]
    index = torch.arange(B, device="cuda") % n
    small = torch.from_numpy(c.y.copy()).to(dtype).cuda()
    y = small[index].contiguous()
    if pack.served(dtype):
        want = ops.soft_cost_raw(y, pack, True)
    else:
        assert pack.stream_served(dtype)
        base = ops.soft_cost_raw(small, pack, True, kernel="stream")          # (one pass: test_batches holds it to the reference)
        want = tuple(t[index] for t in base)
    assert bool((want[0] > 0).any()) and bool(want[3].any())
    for window, nw in _parity_windows(c.arrays, dtype_name):
        what = f"{name} {dtype_name} B={B} window {window} ({nw} windows)"
        assert pack.stream_served(dtype, window), what
        assert _all_same(ops.soft_cost_raw(y, pack, True, kernel="stream"), want), what
        assert _all_same(ops.soft_cost_raw(y, pack, False, kernel="stream")[:3], want[:3]), what


# ---- 3 raw ABI

@pytest.mark.parametrize("name,dtype_name", [("corridor_k12", "float32"), ("corridor_k12", "float64"), ("c3", "float64")])
def test_raw_abi_against_the_reference(name, dtype_name):
    """Straight through ctypes: caller-owned buffers, a gradient with a row stride of its own, canaries around everything."""
    c = S.beyond_case(name)
    lib, pack, dtype = _lib.load(), _pack(c.arrays), getattr(torch, dtype_name)
    assert pack.stream_served(dtype)
    y = _device_y(c, dtype_name)
    B, k = y.shape[0], c.arrays["k"]
    ldg = k + 5
    cost = torch.full((B + 2,), CANARY, dtype=dtype, device="cuda")
    worst, which = cost.clone(), torch.full((B + 2,), 777, dtype=torch.int32, device="cuda")
    grad = torch.full((B + 2, ldg), CANARY, dtype=dtype, device="cuda")
    assert _abi(pack, dtype_name, y, B, y.stride(0), cost[1:], worst[1:], which[1:], grad[1:], ldg) == 0
    _check(c, dtype_name, cost[1:B + 1], worst[1:B + 1], which[1:B + 1], grad[1:B + 1, :k], f"{name} {dtype_name} stream abi")
    for t in (cost, worst, grad):
        assert float(t[0].flatten()[0]) == CANARY and float(t[B + 1].flatten()[0]) == CANARY
    assert int(which[0]) == 777 and int(which[B + 1]) == 777
    assert bool((grad[:, k:] == CANARY).all()) and bool((grad[0] == CANARY).all()) and bool((grad[B + 1] == CANARY).all())
    # argument checks and B = 0
    fn = lib.rayen_soft_cost_stream_f32 if dtype_name == "float32" else lib.rayen_soft_cost_stream_f64
    assert fn(pack.handle, y.data_ptr(), B, k - 1, cost.data_ptr(), None, None, None, 0, None) == -1
    assert fn(pack.handle, None, 0, k, None, None, None, None, 0, None) == 0
    before = cost.clone()
    assert _abi(pack, dtype_name, y, 0, y.stride(0), cost[1:], None, None, None, 0) == 0 and _same(cost, before)


def test_stream_set_argument_checks_and_refusals():
    lib = _lib.load()
    E_BAD_ARG, E_UNSUPPORTED = -1, _lib.E_UNSUPPORTED
    c = S.corridor_case(31)
    pack = ops.CostPack(c.arrays, torch.cuda.current_device())
    y32 = _device_y(c, "float32")
    # nobody asked yet: nothing is served, a call answers RAYEN_E_UNSUPPORTED
    assert lib.rayen_cost_stream_served(pack.handle, 0) == 0 and lib.rayen_cost_stream_served(pack.handle, 1) == 0
    assert _abi(pack, "float32", y32, 31, y32.stride(0), None, None, None, None, 0) == E_UNSUPPORTED
    for bad in (-16, 8, 24, S.MIN_WINDOW32 + 4, S.DEFAULT_WINDOW + 16):
        assert lib.rayen_cost_stream_set(pack.handle, bad) == E_BAD_ARG, bad
    assert lib.rayen_cost_stream_set(None, 0) == E_BAD_ARG
    assert lib.rayen_cost_stream_served(pack.handle, 0) == 0          # (a refused size builds nothing)
    # a window too small for the largest item: not an error, the precision is unserved
    assert lib.rayen_cost_stream_set(pack.handle, S.MIN_WINDOW32 - 16) == 0
    assert lib.rayen_cost_stream_served(pack.handle, 0) == 0
    assert lib.rayen_cost_stream_served(pack.handle, 1) == int(S.stream_served_by_formula(c.arrays, "float64", S.MIN_WINDOW32 - 16)) == 1
    assert _abi(pack, "float32", y32, 31, y32.stride(0), None, None, None, None, 0) == E_UNSUPPORTED
    small64 = S.smallest_window(c.arrays, "float64")
    assert lib.rayen_cost_stream_set(pack.handle, small64 - 16) == 0 and lib.rayen_cost_stream_served(pack.handle, 1) == 0
    assert lib.rayen_cost_stream_set(pack.handle, 0) == 0
    assert lib.rayen_cost_stream_served(pack.handle, 0) == 1 and lib.rayen_cost_stream_served(pack.handle, 1) == 1
    # outside the envelope at any window: a cone of 65 rows in fp32, k = 65
    cone65 = sweep.tile_case("cone65")
    p65 = _pack(cone65.arrays)
    assert not p65.stream_served(torch.float32) and p65.stream_served(torch.float64)
    y = _device_y(cone65, "float32")
    assert _abi(p65, "float32", y, y.shape[0], y.stride(0), None, None, None, None, 0) == E_UNSUPPORTED
    k65 = sweep.k65_case()
    pk = _pack(k65.arrays)
    for dtype_name in DTYPES:
        assert not pk.stream_served(getattr(torch, dtype_name))
        y = _device_y(k65, dtype_name)
        assert _abi(pk, dtype_name, y, y.shape[0], y.stride(0), None, None, None, None, 0) == E_UNSUPPORTED
    with pytest.raises(ValueError):
        ops.soft_cost_raw(y32, pack, False, kernel="bogus")
    pack.close()


# ---- 4 the module

@pytest.mark.parametrize("kernel", ["stream", "auto"])
def test_module_on_config_3_in_fp64_never_reaches_the_mirror(kernel, monkeypatch):
    c = cost_cases.case("c3")

    def no_mirror(*args, **kwargs):
        raise AssertionError("soft_cost.mirror ran for device tensors of a served set")

    monkeypatch.setattr(soft_cost, "mirror", no_mirror)
    sc = SoftCost(c.cs, kernel=kernel).cuda()
    y = torch.from_numpy(c.y.copy()).cuda().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cost = sc(y)
        cost.sum().backward()
        worst, which = sc.violation(y)
    _check(c, "float64", cost.detach(), worst, which, y.grad, f"c3 float64 module kernel={kernel}")
    assert sc._cost_packs and not sc._unsupported


def test_auto_in_fp32_on_config_3_is_the_resident_kernel():
    c = cost_cases.case("c3")
    y = torch.from_numpy(c.y.copy()).float().cuda()
    outs = []
    for kernel in ("resident", "auto", "stream"):
        sc = SoftCost(c.cs, kernel=kernel).cuda()
        yy = y.clone().requires_grad_(True)
        cost = sc(yy)
        cost.sum().backward()
        outs.append((cost.detach(), yy.grad, *sc.violation(yy)))
        if kernel == "auto":
            pack, _ = sc.cost_pack(y.device)
            assert pack.served(torch.float32) and sc._route(pack, torch.float32) == "resident"
            assert sc._route(pack, torch.float64) == "stream"
    assert _all_same(outs[1], outs[0]) and _all_same(outs[2], outs[0])


@pytest.mark.eager_detour
def test_default_module_on_config_3_in_fp64_still_warns_once_and_takes_the_mirror(monkeypatch):
    c = cost_cases.case("c3")
    monkeypatch.delenv("RAYEN_STRICT_HIP", raising=False)
    calls = []
    real = soft_cost.mirror
    monkeypatch.setattr(soft_cost, "mirror", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    sc = SoftCost(c.cs).cuda()
    y = torch.from_numpy(c.y.copy()).cuda()
    with pytest.warns(RuntimeWarning, match="no HIP kernel serves"):
        cost = sc(y)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        again = sc(y)
    assert len(calls) == 2 and torch.equal(cost, again)
    assert (y.device.index, torch.float64, "resident") in sc._unsupported
    # the refusals are kept per route: a module on kernel='stream' whose pack serves nothing at fp64 (its window forced below
    # a quadratic of 64 rows) says so once for itself, remembers (device, dtype, 'stream') and runs the mirror
    st = SoftCost(c.cs, kernel="stream").cuda()
    pack, _ = st.cost_pack(y.device)
    assert not pack.stream_served(torch.float64, S.smallest_window(c.arrays, "float64") - 16)
    del calls[:]
    with pytest.warns(RuntimeWarning, match="no HIP kernel serves"):
        cost_st = st(y)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        again_st = st(y)
    assert len(calls) == 2 and torch.equal(cost_st, again_st) and torch.equal(cost_st, cost)
    assert st._unsupported == {(y.device.index, torch.float64, "stream")}
    assert sc._unsupported == {(y.device.index, torch.float64, "resident")}
    monkeypatch.setenv("RAYEN_STRICT_HIP", "1")
    with pytest.raises(_lib.RayenError):
        ops.soft_cost_raw(y, pack, False, kernel="stream")
    k65 = sweep.k65_case()
    with pytest.raises(_lib.RayenError):
        ops.soft_cost_raw(_device_y(k65, "float64"), _pack(k65.arrays), False, kernel="stream")


def test_fused_cost_computer_on_the_streamed_route():
    c = cost_cases.case("k17_m33")
    y = torch.from_numpy(c.y.copy()).float().cuda().unsqueeze(2).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loss = CostComputer(c.cs, fused=True, kernel="stream").cuda().getSumSoftCostAllSamples(y)
        loss.backward()
    plain = CostComputer(c.cs).cuda()
    y2 = y.detach().clone().requires_grad_(True)
    want = plain.getSumSoftCostAllSamples(y2)
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-4 * abs(want.item())
    assert torch.allclose(y.grad, y2.grad, rtol=1e-3, atol=1e-4 * float(y2.grad.abs().max()))


# ---- 5 with an LMI: the streamed rows, then the launch of rayen_cost_lmi.hip on the same stream

def test_streamed_rows_then_the_lmi_launch():
    c = S.lmi_case()
    pack = _pack(c.arrays)
    assert not pack.served(torch.float32) and pack.stream_served(torch.float32)
    y = torch.from_numpy(c.y.copy()).float().cuda()
    cost, worst, which, grad = ops.soft_cost_raw(y, pack, True, kernel="stream")
    host = lambda *ts: tuple(t.detach().cpu().numpy() for t in ts)          # noqa: E731
    ref = L.check(c, "float32", *host(cost, worst, which, grad), "lin700_lmi20 float32 stream")
    ok = c.finite
    assert (ref["which"][ok] == ref["lmi_id"]).any() and (ref["which"][ok] < ref["lmi_id"]).any()
    # the accumulating launch adds and never overwrites: the result is the streamed rows alone combined on the host with
    # the LMI alone, exactly (tests/test_gpu_soft_cost_lmi.py::test_mixed_set_is_the_rows_launch_plus_the_lmi_alone)
    rows = _pack(c.rows_arrays)
    assert rows.stream_served(torch.float32)
    rcost, rworst, rwhich, rgrad = ops.soft_cost_raw(y, rows, True, kernel="stream")
    lcost, lworst, _, lgrad = ops.soft_cost_raw(y, _pack(c.alone_arrays), True)
    okd = torch.from_numpy(ok).cuda()
    assert torch.equal(cost[okd], (rcost + lcost)[okd]) and torch.equal(grad[okd], (rgrad + lgrad)[okd])
    lmi_wins = (lworst > rworst) | ((lworst == rworst) & (rwhich >= ref["lmi_id"]))
    assert torch.equal(worst[okd], torch.where(lmi_wins, lworst, rworst)[okd])
    assert torch.equal(which[okd], torch.where(lmi_wins, torch.full_like(rwhich, ref["lmi_id"]), rwhich)[okd])
    assert bool((lcost[okd] > 0).any()) and bool((lcost[okd] == 0).any()) and bool((rcost[okd] > 0).any())
    cost0, worst0, which0, none = ops.soft_cost_raw(y, pack, False, kernel="stream")
    assert none is None and _all_same((cost0, worst0, which0), (cost, worst, which))
