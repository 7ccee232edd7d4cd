"""Sweep of the soft-cost kernels (rayen_amd/csrc/rayen_cost.hip) over every instantiation, path, edge and limit, against the
fp64 reference and the bars of tests/cost_reference.py (unchanged: ``(d + 8) u S``, fp32 inputs re-referenced after rounding,
no sample excluded).  The cases are tests/cost_sweep_cases.py; tests/test_soft_cost_sweep_host.py shows on the host that they
are sound.

The ten kernel instantiations and the case that launches each:

    cost_mfma_kernel<true>          every fp32 case with a gradient, first test_width_op[float32-*]
    cost_mfma_kernel<false>         the values-only repeat of test_width_op[float32-*]
    cost_lane64_kernel<8, true>     test_width_op[float64-k] for k = 1, 4, 8
    cost_lane64_kernel<8, false>    its values-only repeat
    cost_lane64_kernel<16, true>    test_width_op[float64-k] for k = 9, 16       (test_row_tiles, k = 12, too)
    cost_lane64_kernel<16, false>   its values-only repeat
    cost_lane64_kernel<32, true>    test_width_op[float64-k] for k = 17, 32
    cost_lane64_kernel<32, false>   its values-only repeat
    cost_lane64_kernel<64, true>    test_width_op[float64-k] for k = 33, 36, 60, 63, 64
    cost_lane64_kernel<64, false>   its values-only repeat

``RAYEN_COST_SWEEP_REPORT=<file>`` writes the largest gap/bar per family and precision there when the module is done (a record
of the room under the bars, not a bar)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cost_reference                                         # noqa: E402
import cost_sweep_cases as sweep                              # noqa: E402
from helpers import COST_RATIOS, COST_U                       # noqa: E402
from helpers import cost_check as _check                      # noqa: E402
from helpers import cost_device_y as _device_y                # noqa: E402
from rayen_amd import _lib, ops                               # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ["float32", "float64"]
CANARY = 12345.0
_PACKS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("RAYEN_COST_SWEEP_REPORT")
    if path:
        with open(path, "w") as out:
            out.write("largest gap/bar of the soft-cost sweep per family and precision (<= 1 by construction of the bars)\n")
            for (family, dtype_name), ratio in sorted(COST_RATIOS.items()):
                out.write(f"{family:8s} {dtype_name:8s} {ratio:.3f}\n")


def _pack(c):
    key = id(c.arrays)
    if key not in _PACKS:
        _PACKS[key] = (c.arrays, ops.CostPack(c.arrays, torch.cuda.current_device()))
    return _PACKS[key][1]


def _same(a, b):
    """Bit for bit, NaNs included."""
    if a.dtype.is_floating_point:
        ints = torch.int32 if a.dtype == torch.float32 else torch.int64
        return torch.equal(a.contiguous().view(ints), b.contiguous().view(ints))
    return torch.equal(a, b)


def _abi(pack, dtype_name, y, B, ld, cost, worst, which, grad, ldg):
    """One call of the C ABI on raw addresses (tensors or None); returns the code, synchronised."""
    fn = _lib.load().rayen_soft_cost_f32 if dtype_name == "float32" else _lib.load().rayen_soft_cost_f64
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    code = fn(pack.handle, ptr(y), B, ld, ptr(cost), ptr(worst), ptr(which), ptr(grad), ldg,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code


def _outputs(dtype, B):
    """cost, worst, which with a canary row on either side."""
    return (torch.full((B + 2,), CANARY, dtype=dtype, device="cuda"), torch.full((B + 2,), CANARY, dtype=dtype, device="cuda"),
            torch.full((B + 2,), 777, dtype=torch.int32, device="cuda"))


def _edges_intact(B, *outs):
    return all(float(t[0]) == (777 if t.dtype == torch.int32 else CANARY) and float(t[B + 1]) == float(t[0]) for t in outs)


def _laid_out(dtype, B, k, kind, fill):
    """``(flat, rows)``: a flat buffer of ``fill`` and the ``[B, k]`` view of it with the layout ``kind`` of
    cost_sweep_cases.layout (rows apart from the buffer's ends, padding columns between them)."""
    off, ld = sweep.layout(kind, k)
    lead = (ld + 3) // 4 * 4
    flat = torch.full((lead + off + B * ld + 8,), fill, dtype=dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0
    rows = flat.as_strided((B, k), (ld, 1), lead + off)
    assert (rows.data_ptr() % 16 == 0) == (off == 0) and rows.stride(0) == ld
    return flat, rows


# ---- 1 width sweep: every K of the fp64 kernel in both variants, both sides of each cut-over; 16-byte pieces partly full

@pytest.mark.parametrize("k", sweep.WIDTHS)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_width_op(dtype_name, k):
    c = sweep.width_case(k)
    pack = _pack(c)
    assert pack.served(getattr(torch, dtype_name))
    pack_id = ops.register_pack(pack)
    y = _device_y(c, dtype_name).requires_grad_(True)
    cost, worst, which, grad = torch.ops.rayen_amd.soft_cost(y, pack_id, True)
    ref = _check(c, dtype_name, cost.detach(), worst, which, grad, f"{c.name} {dtype_name} op", family="width")
    go = torch.from_numpy(np.random.default_rng(5).uniform(0.5, 2.0, size=cost.shape[0])).to(cost.dtype).cuda()
    (gy,) = torch.autograd.grad(cost, y, go)
    u = COST_U[dtype_name]
    _, _, dgrad = cost_reference.bounds(ref, u)
    gon = go.cpu().numpy().astype(np.float64)[:, None]
    got = gy.cpu().numpy().astype(np.float64)
    assert got.shape == (sweep.WIDTH_B, k)
    assert np.all(np.abs(got - gon * ref["grad"]) <= gon * (dgrad + u * np.abs(ref["grad"])))
    # values alone (grad = NULL, the other kernel variant): bit for bit; and a second call repeats the first
    cost0, worst0, which0, none = ops.soft_cost_raw(y.detach(), pack, False)
    assert none is None
    cost2, worst2, which2, grad2 = ops.soft_cost_raw(y.detach(), pack, True)
    for a, b in ((cost0, cost), (worst0, worst), (which0, which), (cost2, cost), (worst2, worst), (which2, which), (grad2, grad)):
        assert _same(a, b.detach())


@pytest.mark.parametrize("k", sweep.WIDTHS)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_width_abi(dtype_name, k):
    """Caller-owned buffers: y with NaN padding columns (row stride k + 3), a gradient with a row stride of its own."""
    c = sweep.width_case(k)
    pack, dtype, B, ldg = _pack(c), getattr(torch, dtype_name), sweep.WIDTH_B, k + 5
    wide = torch.full((B, k + 3), float("nan"), dtype=dtype, device="cuda")
    wide[:, :k] = torch.from_numpy(c.y.copy()).to(dtype)
    cost, worst, which = _outputs(dtype, B)
    grad = torch.full((B + 2, ldg), CANARY, dtype=dtype, device="cuda")
    assert _abi(pack, dtype_name, wide, B, k + 3, cost[1:], worst[1:], which[1:], grad[1:], ldg) == 0
    _check(c, dtype_name, cost[1:B + 1], worst[1:B + 1], which[1:B + 1], grad[1:B + 1, :k], f"{c.name} {dtype_name} abi", family="width")
    assert _edges_intact(B, cost, worst, which)
    assert bool((grad[:, k:] == CANARY).all()) and bool((grad[0] == CANARY).all()) and bool((grad[B + 1] == CANARY).all())
    cost0, worst0, which0 = _outputs(dtype, B)
    assert _abi(pack, dtype_name, wide, B, k + 3, cost0[1:], worst0[1:], which0[1:], None, 0) == 0
    assert _same(cost0, cost) and _same(worst0, worst) and _same(which0, which)


# ---- 2 alignment: the 16-byte loads and stores against their scalar fallbacks, independently for y and grad

@pytest.mark.parametrize("dtype_name,k", [(d, k) for d in DTYPES for k in sweep.ALIGN_WIDTHS[d]])
def test_alignment_matrix(dtype_name, k):
    c = sweep.width_case(k)
    pack, dtype, B = _pack(c), getattr(torch, dtype_name), sweep.WIDTH_B
    data = torch.from_numpy(c.y.copy()).to(dtype).cuda()
    first = None
    for y_kind in sweep.LAYOUTS:
        for g_kind in sweep.LAYOUTS:
            yflat, y = _laid_out(dtype, B, k, y_kind, float("nan"))
            y.copy_(data)
            gflat, grad = _laid_out(dtype, B, k, g_kind, CANARY)
            cost, worst, which = _outputs(dtype, B)
            assert _abi(pack, dtype_name, y, B, y.stride(0), cost[1:], worst[1:], which[1:], grad, grad.stride(0)) == 0
            what = f"{c.name} {dtype_name} y {y_kind} grad {g_kind}"
            _check(c, dtype_name, cost[1:B + 1], worst[1:B + 1], which[1:B + 1], grad, what, family="width")
            got = (cost.clone(), worst.clone(), which.clone(), grad.clone())
            assert _edges_intact(B, cost, worst, which), what
            grad.fill_(CANARY)                     # (what was written is kept in `got`: nothing else may have been)
            assert bool((gflat == CANARY).all()), what
            if first is None:
                first = got
            assert all(_same(a, b) for a, b in zip(got, first)), what
            # the values-only variant reads y the same way
            cost0, worst0, which0 = _outputs(dtype, B)
            assert _abi(pack, dtype_name, y, B, y.stride(0), cost0[1:], worst0[1:], which0[1:], None, 0) == 0
            assert _same(cost0, first[0]) and _same(worst0, first[1]) and _same(which0, first[2]), what


def test_column_offset_view_through_the_op():
    """k = 36 columns of a wider tensor, starting at its column 1: a vectorisable k on rows that are not 16-byte aligned."""
    c = sweep.width_case(36)
    pack = _pack(c)
    data = torch.from_numpy(c.y.copy()).float().cuda()
    wide = torch.full((sweep.WIDTH_B, 44), float("nan"), device="cuda")
    wide[:, 1:37] = data
    view = wide[:, 1:37]
    assert view.data_ptr() % 16 == 4 and view.stride(0) == 44
    cost, worst, which, grad = torch.ops.rayen_amd.soft_cost(view, ops.register_pack(pack), True)
    _check(c, "float32", cost, worst, which, grad, f"{c.name} float32 column-offset view", family="width")
    want = ops.soft_cost_raw(data, pack, True)
    assert all(_same(a, b) for a, b in zip((cost, worst, which, grad), want))


# ---- 3 row tiles, 4 every index reportable

@pytest.mark.parametrize("name", list(sweep.TILE_SETS))
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_row_tiles(dtype_name, name):
    c = sweep.tile_case(name)
    pack = _pack(c)
    y = _device_y(c, dtype_name)
    if dtype_name == "float32" and name in sweep.TILE_REFUSED32:
        assert not pack.served(torch.float32) and pack.served(torch.float64)
        with pytest.raises(_lib.RayenError) as err:
            ops.soft_cost_raw(y, pack, True)
        assert err.value.code == _lib.E_UNSUPPORTED
        return
    assert pack.served(getattr(torch, dtype_name))
    cost, worst, which, grad = ops.soft_cost_raw(y, pack, True)
    _check(c, dtype_name, cost, worst, which, grad, f"{c.name} {dtype_name}", family="tiles")
    cost0, worst0, which0, _ = ops.soft_cost_raw(y, pack, False)
    assert _same(cost0, cost) and _same(worst0, worst) and _same(which0, which)


@pytest.mark.parametrize("name", sweep.COVERAGE)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_every_index_is_reported(dtype_name, name):
    """One row per stacked index of which that index is the decided worst (the host test asserts the coverage): a wrong id0
    of any tile, or a wrong row within one, shows."""
    c = sweep.coverage_case(name)
    cost, worst, which, grad = ops.soft_cost_raw(_device_y(c, dtype_name), _pack(c), True)
    ref = _check(c, dtype_name, cost, worst, which, grad, f"{c.name} {dtype_name}", family="tiles")
    want = [j for j in range(sweep.n_values(c.arrays)) if j not in sweep.COVERAGE_UNREACHABLE[name]]
    assert which.cpu().numpy().tolist() == ref["which"].tolist() == want


# ---- 5 batch geometry

@pytest.mark.parametrize("dtype_name", DTYPES)
def test_batch_heads_repeat_the_long_run(dtype_name):
    c = sweep.batch_case()
    pack = _pack(c)
    y = _device_y(c, dtype_name)
    full = ops.soft_cost_raw(y, pack, True)
    _check(c, dtype_name, *full, f"{c.name} {dtype_name} B=257", family="batch")
    for B in sweep.BATCHES:
        head = ops.soft_cost_raw(y[:B].clone(), pack, True)
        assert all(_same(a, b[:B]) for a, b in zip(head, full)), B
        head0 = ops.soft_cost_raw(y[:B].clone(), pack, False)
        assert all(_same(a, b[:B]) for a, b in zip(head0[:3], full)), B


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_second_round_of_the_persistent_loop(dtype_name):
    """One group more than the resident waves take in a round (and a partial last group): the per-group reset of the
    accumulators.  Checked in full against the reference; the first 257 rows also bit for bit against a launch of their own."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    c = sweep.rounds_case(sweep.rounds_batch(cus, dtype_name))
    pack = _pack(c)
    y = _device_y(c, dtype_name)
    full = ops.soft_cost_raw(y, pack, True)
    _check(c, dtype_name, *full, f"{c.name} {dtype_name}", family="batch")
    head = ops.soft_cost_raw(y[:257].clone(), pack, True)
    assert all(_same(a, b[:257]) for a, b in zip(head, full))
    values = ops.soft_cost_raw(y, pack, False)
    assert all(_same(a, b) for a, b in zip(values[:3], full))


# ---- 6 exact cases

@pytest.mark.parametrize("name", list(sweep.EXACT))
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_exact_cases(dtype_name, name):
    c = sweep.EXACT[name]()
    cost, worst, which, grad = ops.soft_cost_raw(_device_y(c, dtype_name), _pack(c), True)
    ref = _check(c, dtype_name, cost, worst, which, grad, f"{c.name} {dtype_name}")
    cost, worst, grad = (t.cpu().numpy().astype(np.float64) for t in (cost, worst, grad))
    which = which.cpu().numpy()
    rows = {"ties": slice(None), "zero": slice(None), "apex": list(sweep.APEX_ROWS) + [3], "lone_lane": slice(None)}[name]
    assert np.array_equal(which[rows], ref["which"][rows])                # (ties: the lowest index, as the reference's argmax)
    assert np.array_equal(cost[rows], ref["cost"][rows]) and np.array_equal(worst[rows], ref["worst"][rows])
    assert np.array_equal(grad[rows], ref["grad"][rows])
    if name == "ties":
        assert [int(which[s]) for s, _, _ in sweep.TIES] == [low for _, low, _ in sweep.TIES]
    if name == "zero":
        z = list(sweep.ZERO_ROWS)
        assert not np.any(cost[z]) and not np.any(worst[z]) and not np.any(grad[z])
    if name == "apex":
        a, r = c.arrays, list(sweep.APEX_ROWS)
        g = -(c.y[r] @ a["c"][0]) - a["d"][0]
        assert np.array_equal(grad[r], -2.0 * g[:, None] * a["c"][0][None, :]) and np.array_equal(cost[r], g * g)
    if name == "lone_lane":
        assert np.flatnonzero(cost).tolist() == [17] and np.flatnonzero(np.any(grad != 0, axis=1)).tolist() == [17]
    values = ops.soft_cost_raw(_device_y(c, dtype_name), _pack(c), False)
    assert np.array_equal(values[0].cpu().numpy(), cost) and np.array_equal(values[2].cpu().numpy(), which)


# ---- 7 NaN placement

@pytest.mark.parametrize("dtype_name", DTYPES)
def test_nan_placement(dtype_name):
    clean_case = sweep.width_case(sweep.NAN_K)
    pack = _pack(clean_case)
    clean = ops.soft_cost_raw(_device_y(clean_case, dtype_name), pack, True)
    for col in sweep.NAN_COLS:
        for row in sweep.NAN_ROWS:
            c = sweep.nan_case(col, row)
            got = ops.soft_cost_raw(_device_y(c, dtype_name), pack, True)
            _check(c, dtype_name, *got, f"{c.name} {dtype_name}")
            cost, worst, which, grad = got
            assert bool(torch.isnan(cost[row])) and bool(torch.isnan(worst[row])) and int(which[row]) == -1
            assert bool(torch.isnan(grad[row]).all())
            keep = torch.arange(sweep.WIDTH_B, device="cuda") != row
            assert all(_same(a[keep], b[keep]) for a, b in zip(got, clean)), (col, row)
            values = ops.soft_cost_raw(_device_y(c, dtype_name), pack, False)
            assert all(_same(a, b) for a, b in zip(values[:3], got)), (col, row)


# ---- 8 limits

@pytest.mark.parametrize("dtype_name", DTYPES)
def test_largest_served_image_and_one_row_over(dtype_name):
    dtype, m = getattr(torch, dtype_name), sweep.limit_rows(dtype_name)
    assert m == {"float32": 608, "float64": 2275}[dtype_name]
    c = sweep.limit_case(m)
    pack = ops.CostPack(c.arrays, torch.cuda.current_device())
    assert pack.served(dtype)
    cost, worst, which, grad = ops.soft_cost_raw(_device_y(c, dtype_name), pack, True)
    _check(c, dtype_name, cost, worst, which, grad, f"{c.name} {dtype_name}", family="limits")
    values = ops.soft_cost_raw(_device_y(c, dtype_name), pack, False)
    assert _same(values[0], cost) and _same(values[1], worst) and _same(values[2], which)
    pack.close()
    over = sweep.limit_case(m + 1)
    pack = ops.CostPack(over.arrays, torch.cuda.current_device())
    assert not pack.served(dtype)
    for want_grad in (True, False):
        with pytest.raises(_lib.RayenError) as err:
            ops.soft_cost_raw(_device_y(over, dtype_name), pack, want_grad)
        assert err.value.code == _lib.E_UNSUPPORTED
    pack.close()


def test_served_follows_the_image_formulas():
    """``served`` of every set of the sweep is what the layout in RayenCostPack's comments gives; and for the fp64 image the
    largest linear-only set at a width on either side of each cut-over of its K (a K one step too large halves it)."""
    for c in [sweep.width_case(k) for k in sweep.WIDTHS] + [sweep.tile_case(n) for n in sweep.TILE_SETS]:
        for d in DTYPES:
            assert _pack(c).served(getattr(torch, d)) == sweep.served_by_formula(c.arrays, d), (c.name, d)
    rng = np.random.default_rng(8)
    for k in (8, 9, 16, 17, 32, 33):
        m = 1
        while sweep.image_bytes64(m + 1, 0, (), 0, k) <= sweep.LDS_BUDGET:
            m += 1
        for rows, served in ((m, True), (m + 1, False)):
            pack = ops.CostPack(sweep.make_set(k, rng.standard_normal((rows, k)), np.ones(rows)), torch.cuda.current_device())
            assert pack.served(torch.float64) == served, (k, rows)
            pack.close()


def test_k65_packs_and_every_call_is_refused():
    c = sweep.k65_case()
    pack = ops.CostPack(c.arrays, torch.cuda.current_device())
    for dtype_name in DTYPES:
        assert not pack.served(getattr(torch, dtype_name))
        for want_grad in (True, False):
            with pytest.raises(_lib.RayenError) as err:
                ops.soft_cost_raw(_device_y(c, dtype_name), pack, want_grad)
            assert err.value.code == _lib.E_UNSUPPORTED
    pack.close()


# ---- 9 optional outputs

@pytest.mark.parametrize("k", [36, 12])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_optional_outputs(dtype_name, k):
    c = sweep.width_case(k) if k == 36 else sweep.tile_case("mixed")
    pack, dtype, B = _pack(c), getattr(torch, dtype_name), c.y.shape[0]
    y = _device_y(c, dtype_name)
    full = _outputs(dtype, B) + (torch.full((B + 2, k), CANARY, dtype=dtype, device="cuda"),)
    assert _abi(pack, dtype_name, y, B, k, full[0][1:], full[1][1:], full[2][1:], full[3][1:], k) == 0
    _check(c, dtype_name, full[0][1:B + 1], full[1][1:B + 1], full[2][1:B + 1], full[3][1:B + 1], f"{c.name} {dtype_name} full")
    # (cost, worst, which, grad) passed
    for passed in ((1, 0, 0, 0), (0, 1, 1, 0), (1, 1, 0, 1), (1, 0, 0, 1), (0, 0, 0, 1), (0, 0, 1, 0)):
        outs = _outputs(dtype, B) + (torch.full((B + 2, k), CANARY, dtype=dtype, device="cuda"),)
        args = [t[1:] if use else None for t, use in zip(outs, passed)]
        assert _abi(pack, dtype_name, y, B, k, *args, k) == 0
        for t, ref_t, use in zip(outs, full, passed):
            if use:
                assert _same(t, ref_t), passed
            else:
                assert bool((t == (777 if t.dtype == torch.int32 else CANARY)).all()), passed


# ---- beyond the bars: an infinite input (the zero padding rows of a cone's tiles must stay out of its norm: 0 x inf = NaN)

@pytest.mark.parametrize("dtype_name", DTYPES)
def test_infinite_input_gives_an_infinite_cost(dtype_name):
    y, a = sweep.inf_case()
    pack = ops.CostPack(a, torch.cuda.current_device())
    rows = list(sweep.INF_ROWS)
    clean = y.copy()
    clean[rows, 3] = 0.0
    to = lambda arr: torch.from_numpy(arr.copy()).to(getattr(torch, dtype_name)).cuda()          # noqa: E731
    want = ops.soft_cost_raw(to(clean), pack, True)
    for want_grad in (True, False):
        cost, worst, which, grad = ops.soft_cost_raw(to(y), pack, want_grad)
        assert bool(torch.isinf(cost[rows]).all()) and bool((cost[rows] > 0).all()), cost[rows]
        assert bool(torch.isinf(worst[rows]).all()) and bool((worst[rows] > 0).all()) and which[rows].tolist() == [0, 0]
        keep = torch.ones(y.shape[0], dtype=torch.bool, device="cuda")
        keep[rows] = False
        got = (cost, worst, which) + ((grad,) if want_grad else ())
        assert all(_same(g[keep], w[keep]) for g, w in zip(got, want))
    pack.close()
