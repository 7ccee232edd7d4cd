"""Round 9 of the W-in-LDS schedule of the f16-pair forward (rayen_amd/csrc/rayen_mfma_pair_wl.hip, "Drain"): with
rayen_pair_drain(1) a wave's issue priority follows its progress (down with every further group it claims, down twice more
inside its last group), the screening instances take a row's NaN / Inf flag from ||sv v||^2 instead of folding its f16 pieces,
and the half-to-half sums and maxima go through v_permlane32_swap instead of LDS.  None of it may change a bit: y, kappa and
the arg-max record under drain mode 1 equal those under mode 0 and those of the plain schedule (rayen_pair_schedule(0)); the
NaN flag and y on rows carrying NaN, +Inf, -Inf, 1e+-20 and zeros, placed in the first and in the last group, equal those of
the instances without screening (rayen_pair_screen(0), which keep pair_nan_fold); the screening counters under mode 1 stay
sound (no more skips than groups, none for a segment that cannot be screened) and equal those of mode 0, since a skip depends
on a group's rows alone.  Batches: 1, 31, 33, 511, 512, 513 (fewer than, exactly and more than sixteen groups), 32 16 2 4 + 5
(two groups for each of 128 waves and a ragged last one) and, so that waves of one workgroup do claim second and third groups
whatever the number of compute units, 262 144 + 5.  Needs an MI355X."""
import ctypes
import os

import pytest
import torch

from rayen_amd import _lib, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

pytestmark = pytest.mark.gpu

BATCHES = [1, 31, 33, 511, 512, 513, 32 * 16 * 2 * 4 + 5, 262144 + 5]
SETS = ["c3", "n64_many_aux"]


def _raw(name):
    if name == "c3":
        return workloads.make_raw("c3", seed=7)
    return workloads.random_lin_quad_soc(k=64, m=32, n_quad=5, n_soc=3, seed=25)


_PACKS = {}


def _pack(name):
    """Created with RAYEN_PAIR_SCREEN_GATE=0: every qualifying segment is decided and probed (more skips to get wrong)."""
    if name not in _PACKS:
        cs = workloads.build_constraints(_raw(name))
        prev = os.environ.get("RAYEN_PAIR_SCREEN_GATE")
        os.environ["RAYEN_PAIR_SCREEN_GATE"] = "0"
        try:
            layer = ConstraintModule(cs, method="RAYEN", create_map=False).to("cuda")
            dp, _ = layer.device_pack(torch.device("cuda", torch.cuda.current_device()))
        finally:
            if prev is None:
                del os.environ["RAYEN_PAIR_SCREEN_GATE"]
            else:
                os.environ["RAYEN_PAIR_SCREEN_GATE"] = prev
        assert dp.info().mfma_f32 == 3, "the f16-pair family serves this pack"
        _PACKS[name] = (cs, layer, dp)
    return _PACKS[name]


@pytest.fixture
def lib():
    lib = _lib.load()
    prev = lib.rayen_pair_schedule(3), lib.rayen_pair_screen(-1), lib.rayen_pair_drain(-1)
    yield lib
    lib.rayen_pair_screen_counters(None)
    lib.rayen_pair_drain(prev[2])
    lib.rayen_pair_screen(prev[1])
    lib.rayen_pair_schedule(prev[0])


def _run(lib, dp, v, want_active, schedule=3, screen=1, drain=0, counts=None):
    lib.rayen_pair_schedule(schedule)
    lib.rayen_pair_screen(screen)
    lib.rayen_pair_drain(drain)
    assert (lib.rayen_pair_schedule(-1), lib.rayen_pair_screen(-1), lib.rayen_pair_drain(-1)) == (schedule, screen, drain)
    dp.nan_flag.zero_()
    if counts is not None:
        counts.zero_()
        lib.rayen_pair_screen_counters(ctypes.c_void_p(counts.data_ptr()))
    y, kappa, active = ops.project_raw(v, dp, want_active=want_active)
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


def _plain_rows(B, n, seed):
    return torch.empty(B, n, device="cuda").uniform_(-1.5, 1.5, generator=torch.Generator(device="cuda").manual_seed(seed))


EDGES = ("nan", "+inf", "-inf", "1e20", "1e-20", "zero")


def _edge_rows(B, n, seed):
    """One row of every kind in the first group and one in the last (as many as fit), ordinary rows around them."""
    v = _plain_rows(B, n, seed)
    first = [r for r in (3, 7, 11, 13, 17, 29) if r < B]
    last_lo = ((B - 1) // 32) * 32
    last = [r for r in (B - 1, B - 2, B - 3, B - 4, B - 5, B - 6) if r >= last_lo and r >= 0 and r not in first]
    for rows in (first, last):
        for r, kind in zip(rows, EDGES if B >= 6 else EDGES[:1]):
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


@pytest.mark.parametrize("want_active", [False, True])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", SETS)
def test_drain_mode_changes_no_bit(name, B, want_active, lib):
    cs, layer, dp = _pack(name)
    v = _plain_rows(B, cs.n, 9000 + B)
    y0, k0, a0, f0 = _run(lib, dp, v, want_active, drain=0)
    y1, k1, a1, f1 = _run(lib, dp, v, want_active, drain=1)
    yp, kp, ap, fp = _run(lib, dp, v, want_active, schedule=0)
    assert _same(y1, y0) and _same(k1, k0) and _same(y1, yp) and _same(k1, kp)
    assert f0 == f1 == fp == 0
    if want_active:
        assert torch.equal(a1, a0) and torch.equal(a1, ap)


@pytest.mark.parametrize("drain", [0, 1])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", SETS)
def test_flag_and_y_on_edge_rows_equal_the_unscreened_instances(name, B, drain, lib):
    """nan_row from ||sv v||^2 (screening instances) against pair_nan_fold (rayen_pair_screen(0)): the same flag, the same y."""
    cs, layer, dp = _pack(name)
    v = _edge_rows(B, cs.n, 700 + B)
    y0, k0, a0, f0 = _run(lib, dp, v, True, screen=0, drain=0)
    y1, k1, a1, f1 = _run(lib, dp, v, True, screen=1, drain=drain)
    assert f0 == f1 == 1, (f0, f1)      # (every batch carries at least the NaN row)
    assert _same(y1, y0) and _same(k1, k0) and torch.equal(a1, a0)
    # the flag is the rows': without the non-finite rows it is clear on both paths
    finite = torch.isfinite(v).all(dim=1)
    if bool(finite.any()):
        vf = v[finite].contiguous()
        assert _run(lib, dp, vf, False, screen=0, drain=0)[3] == 0
        assert _run(lib, dp, vf, False, screen=1, drain=drain)[3] == 0


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", SETS)
def test_counters_under_drain_stay_sound(name, B, lib):
    cs, layer, dp = _pack(name)
    v = _plain_rows(B, cs.n, 1000 * (B % 997) + 3)
    counts0 = torch.zeros(64, dtype=torch.int32, device="cuda")
    counts1 = torch.zeros(64, dtype=torch.int32, device="cuda")
    _run(lib, dp, v, False, drain=0, counts=counts0)
    _run(lib, dp, v, False, drain=1, counts=counts1)
    groups = (B + 31) // 32
    segs = dp.consts.segments
    c0, c1 = counts0.cpu().tolist(), counts1.cpu().tolist()
    assert c1 == c0, "a skip depends on the group's rows alone, not on the order in which waves issue"
    for i, s in enumerate(segs):
        assert 0 <= c1[i] <= groups
        if s.type not in (_lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC, _lib.SEG_SOC):
            assert c1[i] == 0
    assert all(c == 0 for c in c1[len(segs):])
    assert sum(c1) < groups * len(segs)
