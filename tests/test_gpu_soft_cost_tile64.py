"""The fp64 tile soft cost (rayen_amd/csrc/rayen_cost_tile64.hip: blocks of 16 stacked rows on v_mfma_f64_16x16x4_f64, the
image through LDS in windows) through ``ops.soft_cost_raw(kernel='tile64')``, ``rayen_amd::soft_cost_tile64``, the raw C ABI
and the modules.

Every result is held to the fp64 reference of tests/cost_reference.py by ``helpers.cost_check(c, 'float64', ...)`` at its
existing bars (they hold for any summation order).  The bit contract -- a row's bits depend on the set and on that row's
input alone -- is ``torch.equal`` on integer views.  The cases are tests/cost_cases.py, cost_sweep_cases.py,
cost_stream_cases.py, cost_lmi_cases.py and cost_tile64_cases.py; tests/test_cost_tile64_host.py checks the layout header and
the lane map on the host."""
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
import cost_tile64_cases as T                                 # noqa: E402
from helpers import cost_check as _check                      # noqa: E402
from helpers import cost_device_y as _device_y                # noqa: E402
from rayen_amd import _lib, ops, soft_cost                    # noqa: E402
from rayen_amd.cost_computer import CostComputer              # noqa: E402
from rayen_amd.soft_cost import SoftCost                      # noqa: E402

pytestmark = pytest.mark.gpu
F64 = "float64"
CANARY = 12345.0
E_BAD_ARG = -1
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


def _abi(pack, y, B, ld, cost, worst, which, grad, ldg):
    """One call of rayen_soft_cost_tile64_f64 on raw addresses (tensors or None); returns the code, synchronised."""
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    code = _lib.load().rayen_soft_cost_tile64_f64(pack.handle, ptr(y), B, ld, ptr(cost), ptr(worst), ptr(which), ptr(grad), ldg,
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code


def _outputs(B):
    """cost, worst, which with a canary row on either side."""
    return (torch.full((B + 2,), CANARY, dtype=torch.float64, device="cuda"),
            torch.full((B + 2,), CANARY, dtype=torch.float64, device="cuda"),
            torch.full((B + 2,), 777, dtype=torch.int32, device="cuda"))


def _edges_intact(B, *outs):
    return all(float(t[0]) == (777 if t.dtype == torch.int32 else CANARY) and float(t[B + 1]) == float(t[0]) for t in outs)


def _laid_out(B, k, kind, fill):
    off, ld = sweep.layout(kind, k)
    lead = (ld + 3) // 4 * 4
    flat = torch.full((lead + off + B * ld + 8,), fill, dtype=torch.float64, device="cuda")
    rows = flat.as_strided((B, k), (ld, 1), lead + off)
    assert rows.stride(0) == ld
    return flat, rows


def _run(c, want_grad=True, window=None):
    """(cost, worst, which, grad) of the case on the tile route; ``window``: a forced window first (None leaves the pack's)."""
    pack = _pack(c.arrays)
    if window is not None:
        assert pack.tile64_served(window), (c.name, window)
    return ops.soft_cost_raw(_device_y(c, F64), pack, want_grad, kernel="tile64")


def _checked(c, what, window=0, family=None):
    """The case at ``window`` against the reference; values alone and a second call repeat the first, bit for bit."""
    got = _run(c, True, window)
    ref = _check(c, F64, *got, f"{c.name} tile64 {what}", family=family)
    values = _run(c, False)
    assert values[3] is None and _all_same(values[:3], got), what
    assert _all_same(_run(c, True), got), what
    return got, ref


# ---- 1 against the reference: the sets of the soft-cost tests, every width, row tiles, coverage, exact cases

@pytest.mark.parametrize("name", cost_cases.NAMES)
def test_named_cases(name):
    """Config 3 (``c3``, ``c3_inside``: 512 rows of 64 columns, 256 KiB of image) included, which the resident fp64 kernel refuses."""
    c = cost_cases.case(name)
    pack = _pack(c.arrays)
    assert pack.tile64_served() == T.served_by_formula(c.arrays) is True
    _checked(c, "default window")


@pytest.mark.parametrize("k", sweep.WIDTHS)
def test_widths_through_the_op_and_the_abi(k):
    """Both sides of every instance cut-over (K = 8 | 16 | 32 | 64), column blocks of the gradient partly full; through the op
    with autograd, and through the ABI on caller-owned buffers: y with NaN padding columns, a gradient stride of its own."""
    c = sweep.width_case(k)
    pack = _pack(c.arrays)
    assert pack.tile64_served()
    y = _device_y(c, F64).requires_grad_(True)
    cost, worst, which, grad = torch.ops.rayen_amd.soft_cost_tile64(y, ops.register_pack(pack), True)
    _check(c, F64, cost.detach(), worst, which, grad, f"{c.name} tile64 op")
    go = torch.from_numpy(np.random.default_rng(5).uniform(0.5, 2.0, size=cost.shape[0])).cuda()
    (gy,) = torch.autograd.grad(cost, y, go)
    assert gy.shape == (sweep.WIDTH_B, k) and _same(gy, go[:, None] * grad)
    B, ldg = sweep.WIDTH_B, k + 5
    wide = torch.full((B, k + 3), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :k] = y.detach()
    cost1, worst1, which1 = _outputs(B)
    grad1 = torch.full((B + 2, ldg), CANARY, dtype=torch.float64, device="cuda")
    assert _abi(pack, wide, B, k + 3, cost1[1:], worst1[1:], which1[1:], grad1[1:], ldg) == 0
    assert _all_same((cost1[1:B + 1], worst1[1:B + 1], which1[1:B + 1], grad1[1:B + 1, :k]), (cost.detach(), worst, which, grad))
    assert _edges_intact(B, cost1, worst1, which1)
    assert bool((grad1[:, k:] == CANARY).all()) and bool((grad1[0] == CANARY).all()) and bool((grad1[B + 1] == CANARY).all())
    cost0, worst0, which0 = _outputs(B)
    assert _abi(pack, wide, B, k + 3, cost0[1:], worst0[1:], which0[1:], None, 0) == 0
    assert _all_same((cost0, worst0, which0), (cost1, worst1, which1))


@pytest.mark.parametrize("name", list(sweep.TILE_SETS))
def test_row_tiles(name):
    c = sweep.tile_case(name)
    assert _pack(c.arrays).tile64_served() == T.served_by_formula(c.arrays) is True          # (cone65 included)
    _checked(c, "default window")


@pytest.mark.parametrize("name", sweep.COVERAGE)
def test_every_index_is_reported(name):
    """One row per stacked index of which that index is the decided worst: a wrong id0 of any block, or a wrong row within
    one, shows."""
    c = sweep.coverage_case(name)
    (cost, worst, which, grad), ref = _checked(c, "coverage")
    want = [j for j in range(sweep.n_values(c.arrays)) if j not in sweep.COVERAGE_UNREACHABLE[name]]
    assert which.cpu().numpy().tolist() == ref["which"].tolist() == want


@pytest.mark.parametrize("name", list(sweep.EXACT))
def test_exact_cases(name):
    """Small integers: every product and sum is exact in any order, the assertions are equalities (ties go to the lowest
    index, exact zeros inside, the apex of a cone, a lone violating lane in a wave)."""
    c = sweep.EXACT[name]()
    (cost, worst, which, grad), ref = _checked(c, "exact")
    cost, worst, grad = (t.cpu().numpy() for t in (cost, worst, grad))
    which = which.cpu().numpy()
    rows = {"ties": slice(None), "zero": slice(None), "apex": list(sweep.APEX_ROWS) + [3], "lone_lane": slice(None)}[name]
    assert np.array_equal(which[rows], ref["which"][rows])
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


# ---- 2 NaN in every lane group and column block; an infinite input

def test_nan_placement():
    clean_case = sweep.width_case(sweep.NAN_K)
    clean = _run(clean_case)
    for col in T.NAN_COLS:
        for row in T.NAN_ROWS:
            c = T.nan_case(col, row)
            got = _run(c)
            _check(c, F64, *got, f"{c.name} tile64")
            cost, worst, which, grad = got
            assert bool(torch.isnan(cost[row])) and bool(torch.isnan(worst[row])) and int(which[row]) == -1
            assert bool(torch.isnan(grad[row]).all())
            keep = torch.arange(sweep.WIDTH_B, device="cuda") != row
            assert all(_same(a[keep], b[keep]) for a, b in zip(got, clean)), (col, row)
            assert _all_same(_run(c, False)[:3], got), (col, row)


def test_infinite_input_gives_an_infinite_cost():
    """The zero padding rows of a cone's blocks stay out of its norm (0 x inf = NaN)."""
    y, a = sweep.inf_case()
    pack = ops.CostPack(a, torch.cuda.current_device())
    rows = list(sweep.INF_ROWS)
    clean = y.copy()
    clean[rows, 3] = 0.0
    to = lambda arr: torch.from_numpy(arr.copy()).cuda()          # noqa: E731
    want = ops.soft_cost_raw(to(clean), pack, True, kernel="tile64")
    for want_grad in (True, False):
        cost, worst, which, grad = ops.soft_cost_raw(to(y), pack, want_grad, kernel="tile64")
        assert bool(torch.isinf(cost[rows]).all()) and bool((cost[rows] > 0).all()), cost[rows]
        assert bool(torch.isinf(worst[rows]).all()) and bool((worst[rows] > 0).all()) and which[rows].tolist() == [0, 0]
        keep = torch.ones(y.shape[0], dtype=torch.bool, device="cuda")
        keep[rows] = False
        got = (cost, worst, which) + ((grad,) if want_grad else ())
        assert all(_same(g[keep], w[keep]) for g, w in zip(got, want))
    pack.close()


# ---- 3 boundaries and layouts

@pytest.mark.parametrize("name", list(T.BOUNDARY))
def test_row_block_boundaries(name):
    """Runs of 15 .. 33 linear and equality rows; cones of 1 and 16 rows (one block: products kept in registers) and of
    17 .. 65 rows (computed again for the gradient): all served, at the smallest window and at the default."""
    c = T.boundary_case(name)
    assert T.served_by_formula(c.arrays)
    first, _ = _checked(c, "default window")
    assert _all_same(_run(c, True, T.smallest_window(c.arrays)), first)


def test_batch_heads_repeat_the_long_run():
    """1 .. 257 rows: sample blocks of 16 and 32, a workgroup's 128, waves with no live sample that still take every barrier."""
    c = sweep.batch_case()
    pack = _pack(c.arrays)
    assert pack.tile64_served()
    y = _device_y(c, F64)
    full = ops.soft_cost_raw(y, pack, True, kernel="tile64")
    _check(c, F64, *full, f"{c.name} tile64 B=257")
    for B in sweep.BATCHES:
        head = ops.soft_cost_raw(y[:B].clone(), pack, True, kernel="tile64")
        assert _all_same(head, tuple(t[:B] for t in full)), B
        head0 = ops.soft_cost_raw(y[:B].clone(), pack, False, kernel="tile64")
        assert _all_same(head0[:3], tuple(t[:B] for t in full[:3])), B
    # a row alone is the same row inside the 257
    for row in (0, 100, 256):
        alone = ops.soft_cost_raw(y[row:row + 1].clone(), pack, True, kernel="tile64")
        assert _all_same(alone, tuple(t[row:row + 1] for t in full)), row


def test_layouts_for_y_and_grad_independently():
    """Offset bases and a row stride of k + 1, NaN padding around y, canaries around every output."""
    c = sweep.tile_case("mixed")
    pack, k, B = _pack(c.arrays), c.arrays["k"], c.y.shape[0]
    assert pack.tile64_served(T.forced_windows(c.arrays)[1])
    data = torch.from_numpy(c.y.copy()).cuda()
    want = ops.soft_cost_raw(data, pack, True, kernel="tile64")
    _check(c, F64, *want, f"{c.name} tile64 three blocks' window")
    for y_kind in sweep.LAYOUTS:
        for g_kind in sweep.LAYOUTS:
            what = f"y {y_kind} grad {g_kind}"
            _, y = _laid_out(B, k, y_kind, float("nan"))
            y.copy_(data)
            gflat, grad = _laid_out(B, k, g_kind, CANARY)
            cost, worst, which = _outputs(B)
            assert _abi(pack, y, B, y.stride(0), cost[1:], worst[1:], which[1:], grad, grad.stride(0)) == 0, what
            assert _all_same((cost[1:B + 1], worst[1:B + 1], which[1:B + 1], grad), want), what
            assert _edges_intact(B, cost, worst, which), what
            grad.fill_(CANARY)
            assert bool((gflat == CANARY).all()), what


@pytest.mark.parametrize("k", [36, 12])
def test_optional_outputs(k):
    c = sweep.width_case(k) if k == 36 else sweep.tile_case("mixed")
    pack, B = _pack(c.arrays), c.y.shape[0]
    assert pack.tile64_served()
    y = _device_y(c, F64)
    full = _outputs(B) + (torch.full((B + 2, k), CANARY, dtype=torch.float64, device="cuda"),)
    assert _abi(pack, y, B, k, full[0][1:], full[1][1:], full[2][1:], full[3][1:], k) == 0
    _check(c, F64, full[0][1:B + 1], full[1][1:B + 1], full[2][1:B + 1], full[3][1:B + 1], f"{c.name} tile64 full")
    for passed in ((1, 0, 0, 0), (0, 1, 1, 0), (1, 1, 0, 1), (1, 0, 0, 1), (0, 0, 0, 1), (0, 0, 1, 0), (0, 0, 0, 0)):
        outs = _outputs(B) + (torch.full((B + 2, k), CANARY, dtype=torch.float64, device="cuda"),)
        args = [t[1:] if use else None for t, use in zip(outs, passed)]
        assert _abi(pack, y, B, k, *args, k) == 0
        for t, ref_t, use in zip(outs, full, passed):
            if use:
                assert _same(t, ref_t), passed
            else:
                assert bool((t == (777 if t.dtype == torch.int32 else CANARY)).all()), passed


# ---- 4 the bit contract across windows; beyond one window; several passes per workgroup

@pytest.mark.parametrize("name", ["tile_mixed", "tile_three_tiles", "width_k36", "width_k64", "k17_m33", "k8_windows"])
def test_forced_windows_give_equal_bits(name):
    c = {"tile_mixed": lambda: sweep.tile_case("mixed"), "tile_three_tiles": lambda: sweep.tile_case("three_tiles"),
         "width_k36": lambda: sweep.width_case(36), "width_k64": lambda: sweep.width_case(64),
         "k17_m33": lambda: cost_cases.case("k17_m33"), "k8_windows": T.k8_case}[name]()
    first, _ = _checked(c, "default window")
    small, three, _ = T.forced_windows(c.arrays)
    K, its = T.width(c.arrays["k"]), T.items(c.arrays)
    assert len(T.partition(its, K, small)) > 1
    for window in (small, three):
        assert _all_same(_run(c, True, window), first), window
        assert _all_same(_run(c, False)[:3], first), window


@pytest.mark.parametrize("name", ["corridor_k12", "c5_shape", "past_limit64", "c3"])
def test_beyond_one_window_at_the_default(name):
    c = S.beyond_case(name)
    a = c.arrays
    assert len(T.partition(T.items(a), T.width(a["k"]), T.DEFAULT_WINDOW)) > 1
    first, _ = _checked(c, "default window")
    assert _all_same(_run(c, True, T.forced_windows(a)[1]), first)          # the window size moves the cuts, not a bit


def test_several_passes_per_workgroup_at_an_odd_and_an_even_number_of_windows():
    """B just over CUs x 128 at k = 8: every workgroup's second pass prefetches window 0 under the last window's walk; from
    then on the buffer of window 0 alternates when the number of windows is odd and stays when it is even.  The rows of the
    small case repeated: samples do not mix, so the result is the small case's, repeated."""
    c = T.k8_case()
    pack = _pack(c.arrays)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    B, n = 128 * cus + 33, c.y.shape[0]
    index = torch.arange(B, device="cuda") % n
    small = torch.from_numpy(c.y.copy()).cuda()
    y = small[index].contiguous()
    base, _ = _checked(c, "default window")
    want = tuple(t[index] for t in base)
    assert bool((want[0] > 0).any()) and bool(want[3].any())
    for window, nw in T.parity_windows(c.arrays) + [(0, None)]:
        what = f"B={B} window {window} ({nw} windows)"
        assert pack.tile64_served(window), what
        assert _all_same(ops.soft_cost_raw(y, pack, True, kernel="tile64"), want), what
        assert _all_same(ops.soft_cost_raw(y, pack, False, kernel="tile64")[:3], want[:3]), what


# ---- 5 with an LMI: the tile rows, then the launch of rayen_cost_lmi.hip on the same stream

def test_tile_rows_then_the_lmi_launch():
    c = S.lmi_case()
    pack = _pack(c.arrays)
    assert pack.tile64_served()
    y = torch.from_numpy(c.y.copy()).cuda()
    cost, worst, which, grad = ops.soft_cost_raw(y, pack, True, kernel="tile64")
    host = lambda *ts: tuple(t.detach().cpu().numpy() for t in ts)          # noqa: E731
    ref = L.check(c, F64, *host(cost, worst, which, grad), "lin700_lmi20 float64 tile64")
    ok = c.finite
    assert (ref["which"][ok] == ref["lmi_id"]).any() and (ref["which"][ok] < ref["lmi_id"]).any()
    cost0, worst0, which0, none = ops.soft_cost_raw(y, pack, False, kernel="tile64")
    assert none is None and _all_same((cost0, worst0, which0), (cost, worst, which))


@pytest.mark.parametrize("name", L.MIXED)
def test_mixed_sets_with_an_lmi(name):
    c = L.case(name, 67)
    _, arrays, _, _ = L.the_set(name)
    pack = _pack(arrays)
    assert pack.tile64_served()
    y = torch.from_numpy(c.y.copy()).cuda()
    cost, worst, which, grad = ops.soft_cost_raw(y, pack, True, kernel="tile64")
    host = lambda *ts: tuple(t.detach().cpu().numpy() for t in ts)          # noqa: E731
    ref = L.check(c, F64, *host(cost, worst, which, grad), f"{name} float64 tile64")
    assert (ref["which"][c.finite] == ref["lmi_id"]).any()
    assert (ref["which"][c.finite] > ref["lmi_id"]).any() == (ref["n_eq"] > 0)          # (eq_shift: an index after the LMI)
    # two launches: the second compares with the stored worst
    assert _abi(pack, y, 67, y.stride(0), None, None, which, None, 0) == E_BAD_ARG


# ---- 6 refusals

def test_set_argument_checks_and_refusals():
    lib = _lib.load()
    E_UNSUPPORTED = _lib.E_UNSUPPORTED
    c = S.corridor_case(31)
    pack = ops.CostPack(c.arrays, torch.cuda.current_device())
    y = _device_y(c, F64)
    # nobody asked yet: nothing is served, a raw call answers RAYEN_E_UNSUPPORTED
    assert lib.rayen_cost_tile64_served(pack.handle) == 0
    assert _abi(pack, y, 31, y.stride(0), None, None, None, None, 0) == E_UNSUPPORTED
    for bad in (-16, 8, 24, T.smallest_window(c.arrays) + 4, T.DEFAULT_WINDOW + 16):
        assert lib.rayen_cost_tile64_set(pack.handle, bad) == E_BAD_ARG, bad
    assert lib.rayen_cost_tile64_set(None, 0) == E_BAD_ARG
    assert lib.rayen_cost_tile64_served(pack.handle) == 0          # (a refused size builds nothing)
    # an item over a forced window: not an error, the set is unserved
    small = T.smallest_window(c.arrays)
    assert not pack.tile64_served(small - 16) and lib.rayen_cost_tile64_served(pack.handle) == 0
    assert not T.served_by_formula(c.arrays, small - 16)
    assert _abi(pack, y, 31, y.stride(0), None, None, None, None, 0) == E_UNSUPPORTED
    with pytest.raises(_lib.RayenError) as err:
        ops.soft_cost_raw(y, pack, True, kernel="tile64")
    assert err.value.code == E_UNSUPPORTED
    assert lib.rayen_cost_tile64_set(pack.handle, small) == 0 and lib.rayen_cost_tile64_served(pack.handle) == 1
    assert lib.rayen_cost_tile64_set(pack.handle, small) == 0          # (idempotent at equal size)
    assert lib.rayen_cost_tile64_set(pack.handle, 0) == 0 and lib.rayen_cost_tile64_served(pack.handle) == 1
    _check(c, F64, *ops.soft_cost_raw(y, pack, True, kernel="tile64"), "corridor_k12[:31] tile64")
    # argument checks of the call, and B = 0
    k = c.arrays["k"]
    cost = torch.full((33,), CANARY, dtype=torch.float64, device="cuda")
    fn = lib.rayen_soft_cost_tile64_f64
    assert fn(pack.handle, y.data_ptr(), 31, k - 1, cost.data_ptr(), None, None, None, 0, None) == E_BAD_ARG
    assert fn(pack.handle, None, 0, k, None, None, None, None, 0, None) == 0
    assert _abi(pack, y, 0, y.stride(0), cost[1:], None, None, None, 0) == 0 and bool((cost == CANARY).all())
    # fp32 input: no entry point; the binding answers E_UNSUPPORTED before it touches the library
    with pytest.raises(_lib.RayenError) as err:
        ops.soft_cost_raw(y.float(), pack, True, kernel="tile64")
    assert err.value.code == E_UNSUPPORTED
    # k = 65: outside the envelope at any window
    k65 = sweep.k65_case()
    pk = _pack(k65.arrays)
    assert not pk.tile64_served() and not T.served_by_formula(k65.arrays)
    yk = _device_y(k65, F64)
    assert _abi(pk, yk, yk.shape[0], yk.stride(0), None, None, None, None, 0) == E_UNSUPPORTED
    with pytest.raises(ValueError):
        ops.soft_cost_raw(y, pack, False, kernel="bogus")
    pack.close()


# ---- 7 the modules

def test_modules_on_the_corridor_shape_with_autograd(monkeypatch):
    c = S.c5_shape_case()

    def no_mirror(*args, **kwargs):
        raise AssertionError("soft_cost.mirror ran for fp64 device tensors of a served set")

    monkeypatch.setattr(soft_cost, "mirror", no_mirror)
    sc = SoftCost(_set_of(c.arrays), kernel="tile64").cuda()
    assert all(np.array_equal(sc.arrays[n], c.arrays[n]) for n in c.arrays)
    y = torch.from_numpy(c.y.copy()).cuda().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cost = sc(y)
        cost.sum().backward()
        worst, which = sc.violation(y)
    _check(c, F64, cost.detach(), worst, which, y.grad, "c5_shape float64 module kernel=tile64")
    assert sc._cost_packs and not sc._unsupported
    pack, _ = sc.cost_pack(y.device)
    assert sc._route(pack, torch.float64) == "tile64"


def _set_of(a):
    """What ``soft_cost.set_arrays`` reads of a constraint set, from a ``set_arrays``-style dict without an LMI (the hand-made
    sets have no ``ConvexConstraints``)."""
    from types import SimpleNamespace as NS
    ends = np.cumsum(a["soc_rows"])
    socs = [NS(M=a["M"][e - r:e], s=a["s"][e - r:e], c=a["c"][j], d=a["d"][j]) for j, (e, r) in enumerate(zip(ends, a["soc_rows"]))]
    return NS(k=a["k"], has_linear_ineq_constraints=a["b1"].size > 0, has_linear_eq_constraints=a["b2"].size > 0,
              lc=NS(A1=a["A1"], b1=a["b1"], A2=a["A2"], b2=a["b2"]), has_quadratic_constraints=a["r"].size > 0,
              qcs=[NS(P=P, q=q, r=r) for P, q, r in zip(a["P"], a["q"], a["r"])], has_soc_constraints=bool(socs), socs=socs,
              has_lmi_constraints=False)


def test_fused_cost_computer_on_config_3():
    c = cost_cases.case("c3")
    y = torch.from_numpy(c.y.copy()).cuda().unsqueeze(2).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loss = CostComputer(c.cs, fused=True, kernel="tile64").cuda().getSumSoftCostAllSamples(y)
        loss.backward()
    ok = ~np.isnan(c.ref["cost"])
    assert ok.all()
    want, gwant = float(np.sum(c.ref["cost"])), c.ref["grad"]
    assert abs(loss.item() - want) <= 1e-9 * abs(want)
    assert np.allclose(y.grad[:, :, 0].cpu().numpy(), gwant, rtol=1e-9, atol=1e-9 * float(np.abs(gwant).max()))


@pytest.mark.eager_detour
def test_fp32_rows_warn_once_and_take_the_mirror_or_raise_in_strict_mode(monkeypatch):
    c = cost_cases.case("k17_m33")
    monkeypatch.delenv("RAYEN_STRICT_HIP", raising=False)
    calls = []
    real = soft_cost.mirror
    monkeypatch.setattr(soft_cost, "mirror", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    sc = SoftCost(c.cs, kernel="tile64").cuda()
    y64 = torch.from_numpy(c.y.copy()).cuda()
    y32 = y64.float()
    with pytest.warns(RuntimeWarning, match="no HIP kernel serves"):
        cost = sc(y32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        again = sc(y32)
        half = sc(y32.half())          # (16-bit rows are computed in fp32: the same remembered key)
        cost64 = sc(y64)               # fp64 rows still run on the kernel
    assert len(calls) == 3 and _same(cost, again) and half.dtype == torch.float16
    assert sc._unsupported == {(y32.device.index, torch.float32, "tile64")}
    worst, which = sc.violation(y64)
    _check(c, F64, cost64, worst, which, None, "k17_m33 float64 module kernel=tile64")
    monkeypatch.setenv("RAYEN_STRICT_HIP", "1")
    strict = SoftCost(c.cs, kernel="tile64").cuda()
    with pytest.raises(_lib.RayenError) as err:
        strict(y32)
    assert err.value.code == _lib.E_UNSUPPORTED


@pytest.mark.eager_detour
@pytest.mark.parametrize("name", ["k17_m33", "c3"])
def test_the_other_routes_answer_as_before(name, monkeypatch):
    """'resident', 'stream' and 'auto' through the module, before and after the pack built and ran its tile image: bit for bit
    (config 3 in fp64 under 'resident' is the mirror, loudly, as before)."""
    monkeypatch.delenv("RAYEN_STRICT_HIP", raising=False)
    c = cost_cases.case(name)
    y = torch.from_numpy(c.y.copy()).cuda()

    def answers(modules):
        out = []
        for sc in modules:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)          # (c3: the resident fp64 kernel refuses, as before)
                for yy in (y, y.float()):
                    yy = yy.clone().requires_grad_(True)
                    cost = sc(yy)
                    cost.sum().backward()
                    out.append((cost.detach(), yy.grad, *sc.violation(yy)))
        return out

    modules = [SoftCost(c.cs, kernel=kernel).cuda() for kernel in ("resident", "stream", "auto")]
    before = answers(modules)
    routes = [m._route(m.cost_pack(y.device)[0], torch.float64) for m in modules]
    for m in modules:          # the tile image on the very packs the modules use
        pack, _ = m.cost_pack(y.device)
        assert pack.tile64_served()
        _check(c, F64, *ops.soft_cost_raw(y, pack, True, kernel="tile64"), f"{name} tile64 on a module's pack")
    after = answers(modules)
    assert all(_all_same(a, b) for a, b in zip(after, before))
    assert routes == [m._route(m.cost_pack(y.device)[0], torch.float64) for m in modules]
    assert routes == ["resident", "stream", "resident" if name == "k17_m33" else "stream"]
