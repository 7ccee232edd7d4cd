"""Round 10 of the W-in-LDS schedule of the f16-pair forward (rayen_amd/csrc/rayen_mfma_pair_wl.hip): the probe reads operands
of its own instead of overwriting the walk's, the running maximum over both halves is formed once per decision point, the
first two waves of a workgroup request their first rows behind the image's chunks and in front of the workgroup barrier, the
other waves right behind it, and every wave requests a further group's rows at the bottom of the group before, behind its last
store of y.  None of it may change a bit: y, kappa and the arg-max record with the screening modes 1 (spectral test and probe) and 2 (spectral test
alone) equal those of the plain schedule (rayen_pair_schedule(0)) and those of the instances without screening
(rayen_pair_screen(0), which share the new head) -- on batches of 1, 31, 32, 33 rows, one workgroup partly filled, every wave
with exactly one group and a ragged one behind them, waves with two and with three groups and a ragged last one (the grid
narrowed with rayen_reserve_cus, which mfma_pair_wl_forward's grid follows); on config 3, an n = 32 set (NKK = 1), n = 60
(ragged width) and a set whose probed segments of several items are followed by skipped ones; with NaN, +-Inf, 1e+-20 and zero
rows in the first and in the last group; with canaries around a ragged y.  The skip counters must not depend on the call
(equal across repeated calls) and must be non-zero where the probe's own test expects skips.  Needs an MI355X."""
import ctypes

import pytest
import torch

import test_gpu_pair_wl_probe as probe      # (its generators and its pack builder: imported, not edited)
from rayen_amd import _lib, ops, workloads

pytestmark = pytest.mark.gpu

SETS = ["c3", "n32", "n60", "n64_many_aux"]
RESERVED = 128      # compute units left free while the larger batches run: the most rayen_reserve_cus takes


def _raw(name):
    if name == "n60":
        return workloads.random_lin_quad_soc(k=60, m=128, n_quad=3, n_soc=2, seed=24)
    return probe._raw(name)      # c3 at the tests' seed (7); n32; five quadratics + three cones


_PACKS = {}


def _pack(name):
    """Created with RAYEN_PAIR_SCREEN_GATE=0: every qualifying segment is decided and probed, the failing probe's path included."""
    if name not in _PACKS:
        _PACKS[name] = probe._make(_raw(name), gate=False)
    return _PACKS[name]


def _grid():
    """Workgroups of a launch with RESERVED compute units left free (mfma_pair_wl_forward: one per compute unit that is left)."""
    return max(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count - RESERVED, 1)


def _batches():
    g = _grid()
    return {"1": 1, "31": 31, "32": 32, "33": 33,
            "part_of_a_workgroup": 32 * 16 - 5,
            "one_group_per_wave_and_a_ragged_one": 32 * 16 * g + 7,
            "two_and_three_groups_per_wave": 32 * 32 * g + 32 * 3 + 7}      # (128 workgroups: the 131 072 + 32 3 + 7 of the round's plan)


BATCHES = ["1", "31", "32", "33", "part_of_a_workgroup", "one_group_per_wave_and_a_ragged_one", "two_and_three_groups_per_wave"]


@pytest.fixture
def lib():
    lib = _lib.load()
    prev = lib.rayen_pair_schedule(3), lib.rayen_pair_screen(-1), lib.rayen_reserve_cus(RESERVED)
    yield lib
    lib.rayen_pair_screen_counters(None)
    lib.rayen_reserve_cus(prev[2])
    lib.rayen_pair_screen(prev[1])
    lib.rayen_pair_schedule(prev[0])


def _run(lib, dp, v, want_active, schedule=3, screen=1, counts=None, out=None):
    lib.rayen_pair_schedule(schedule)
    lib.rayen_pair_screen(screen)
    assert (lib.rayen_pair_schedule(-1), lib.rayen_pair_screen(-1), lib.rayen_reserve_cus(-1)) == (schedule, screen, RESERVED)
    dp.nan_flag.zero_()
    if counts is not None:
        counts.zero_()
        lib.rayen_pair_screen_counters(ctypes.c_void_p(counts.data_ptr()))
    y, kappa, active = ops.project_raw(v, dp, want_active=want_active, out=out)
    assert lib.rayen_last_forward_kernel() == (_lib.KERNEL_PAIR_WL if schedule == 3 else _lib.KERNEL_PAIR)
    torch.cuda.synchronize()
    if counts is not None:
        lib.rayen_pair_screen_counters(None)
    flag = int(dp.nan_flag.item())
    dp.nan_flag.zero_()
    return y, kappa, active, flag


def _same(a, b):
    # (bit patterns: NaN rows compare equal to themselves)
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


EDGES = ("nan", "+inf", "-inf", "1e20", "1e-20", "zero")


def _rows(B, n, seed, edges):
    v = torch.empty(B, n, device="cuda").uniform_(-1.5, 1.5, generator=torch.Generator(device="cuda").manual_seed(seed))
    if not edges:
        return v
    # one row of every kind in the first group and one in the last (as many as fit)
    first = [r for r in (3, 7, 11, 13, 17, 29) if r < B]
    last_lo = ((B - 1) // 32) * 32
    last = [r for r in (B - 1, B - 2, B - 3, B - 4, B - 5, B - 6) if r >= last_lo and r >= 0 and r not in first]
    for rows in (first, last):
        for r, kind in zip(rows, EDGES):
            if kind == "nan":
                v[r, 5] = float("nan")
            elif kind == "+inf":
                v[r, 0] = float("inf")
            elif kind == "-inf":
                v[r, n - 1] = float("-inf")
            elif kind == "1e20":
                v[r] *= 1e20
            elif kind == "1e-20":
                v[r] *= 1e-20
            else:
                v[r] = 0.0
    return v


_REFS = {}


def _reference(lib, name, batch, edges):
    """(rows, the plain schedule's outputs, the unscreened W-in-LDS instances' outputs): computed once, shared, never written."""
    key = (name, batch, edges)
    if key not in _REFS:
        cs, layer, dp = _pack(name)
        B = _batches()[batch]
        v = _rows(B, cs.n, 77 * SETS.index(name) + B % 1009 + (5000 if edges else 0), edges)
        _REFS[key] = (v, _run(lib, dp, v, True, schedule=0), _run(lib, dp, v, True, screen=0))
    return _REFS[key]


@pytest.mark.parametrize("edges", [False, True], ids=["plain_rows", "edge_rows"])
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", SETS)
def test_head_and_probe_change_no_bit(name, batch, edges, lib):
    cs, layer, dp = _pack(name)
    v, plain, unscreened = _reference(lib, name, batch, edges)
    B = v.shape[0]
    flag_want = 1 if edges else 0      # (every batch with edge rows carries a NaN row)
    assert B == _batches()[batch]
    assert plain[3] == unscreened[3] == flag_want
    assert _same(unscreened[0], plain[0]) and _same(unscreened[1], plain[1]) and torch.equal(unscreened[2], plain[2])
    for mode in (1, 2):
        for want_active in (True, False):      # (the tracking instance and the one the benchmark runs)
            y, k, a, f = _run(lib, dp, v, want_active, screen=mode)
            assert f == flag_want, (mode, want_active, f)
            for ref in (plain, unscreened):
                assert _same(y, ref[0]) and _same(k, ref[1]), (mode, want_active)
                if want_active:
                    assert torch.equal(a, ref[2]), (mode, want_active)


@pytest.mark.parametrize("batch", ["31", "33", "part_of_a_workgroup", "one_group_per_wave_and_a_ragged_one", "two_and_three_groups_per_wave"])
@pytest.mark.parametrize("name", ["c3", "n60"])
def test_nothing_is_written_around_a_ragged_y(name, batch, lib):
    """y is a view into a larger allocation with canaries in front of it, behind it and -- at the ragged width, in a padded
    leading dimension -- beside it; v is a view whose surroundings hold NaN, which must not be seen."""
    cs, layer, dp = _pack(name)
    B = _batches()[batch]
    ld = 64      # (n = 60: four canary columns beside every row; c3: the rows are dense)
    v_all = torch.full((B + 128, ld), float("nan"), device="cuda")
    v_all[64:64 + B, :cs.n] = _rows(B, cs.n, 31 * B + len(name), False)
    y_all = torch.full((B + 128, ld), 777.0, device="cuda")
    v, out = v_all[64:64 + B, :cs.n], y_all[64:64 + B]
    y, kappa, _, flag = _run(lib, dp, v, False, screen=1, out=out)
    assert y.data_ptr() == out.data_ptr() and flag == 0
    assert bool((y_all[:64] == 777.0).all()) and bool((y_all[64 + B:] == 777.0).all()), "rows around the batch were written"
    assert bool((y_all[64:64 + B, cs.k:] == 777.0).all()), "columns beyond a row's width were written"
    assert bool(torch.isfinite(y[:, :cs.k]).all()) and bool(torch.isfinite(kappa).all())
    yp, kp, _, _ = _run(lib, dp, v.contiguous(), False, schedule=0)
    assert _same(y[:, :cs.k].contiguous(), yp) and _same(kappa, kp)


@pytest.mark.parametrize("batch", ["33", "part_of_a_workgroup", "one_group_per_wave_and_a_ragged_one", "two_and_three_groups_per_wave"])
@pytest.mark.parametrize("name", ["c3", "n64_many_aux"])
def test_skip_counters_do_not_depend_on_the_call(name, batch, lib):
    """A skip depends on a group's rows alone -- not on which wave walks the group, when its rows were requested or what the
    probe read before: the counters of repeated calls are equal, sound, and show the skips the probe's own test expects."""
    cs, layer, dp = _pack(name)
    B = _batches()[batch]
    v = _rows(B, cs.n, 1000 + B % 997, False)
    seen = []
    for mode in (1, 2):
        per_call = []
        for _ in range(3):
            counts = torch.zeros(64, dtype=torch.int32, device="cuda")
            _run(lib, dp, v, False, screen=mode, counts=counts)
            per_call.append(counts.cpu().tolist())
        assert per_call[0] == per_call[1] == per_call[2], (mode, per_call)
        seen.append(per_call[0])
    both, bound_only = seen
    groups = (B + 31) // 32
    segs = dp.consts.segments
    for i, s in enumerate(segs):
        assert 0 <= bound_only[i] <= both[i] <= groups, (i, bound_only[i], both[i])
        if s.type not in (_lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC, _lib.SEG_SOC):
            assert both[i] == 0
    assert all(c == 0 for c in both[len(segs):])
    if name == "c3" and groups >= 16:
        # (test_gpu_pair_wl_probe.py: most groups of config 3 skip three of its four quadratics -- with the probe, not without)
        quads = [i for i, s in enumerate(segs) if s.type in (_lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC)]
        assert len(quads) == 4
        for i in quads[1:]:
            assert both[i] > 0, (both, groups)
        assert sum(both) > sum(bound_only)
