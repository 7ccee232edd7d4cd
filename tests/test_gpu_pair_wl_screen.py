"""Screening in the W-in-LDS schedule of the f16-pair forward (rayen_amd/csrc/rayen_mfma_pair_wl.hip, round 7): in front of a
quadratic / cone that owns its tiles the walk bounds the segment's candidate for the 32 samples of a group and skips the
segment's tiles when the bound is below the running maximum of every live sample.  A skip must change NOTHING: y, kappa and
the arg-max record with screening on equal those with screening off (the instances of round 6) bit for bit -- on every set
shape the schedule serves, ragged batches, rows of every magnitude, zero, NaN and infinite rows -- and on a set in which a
cone's candidate crosses the running maximum inside the groups (skipped and walked groups side by side).  So that the
equalities are not vacuous, the counters must report that most groups of config 3 do skip their cones.  Needs an MI355X."""
import ctypes
import os

import pytest
import torch

from rayen_amd import _lib, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

pytestmark = pytest.mark.gpu


def _raw(name):
    if name == "c3":
        return workloads.make_raw("c3", seed=7)
    if name == "c3_cone_half_active":
        # the first cone's block scaled by 4: the fp64 evaluator (rayen_amd/eager.py) has it active on 0.48 of U(-1.5, 1.5) rows
        raw = workloads.make_raw("c3", seed=7)
        raw["M"][0] = raw["M"][0] * 4.0
        return raw
    return {"n64_many_aux": lambda: workloads.random_lin_quad_soc(k=64, m=32, n_quad=5, n_soc=3, seed=25),
            "n32": lambda: workloads.random_lin_quad_soc(k=32, m=300, n_quad=3, n_soc=2, seed=17),
            "n36": lambda: workloads.random_lin_quad_soc(k=36, m=100, n_quad=2, n_soc=1, seed=23)}[name]()


_PACKS = {}


def _pack(name, gate=False):
    """gate=False: the pack is created with RAYEN_PAIR_SCREEN_GATE=0, so EVERY qualifying segment is decided in front of (the
    creation-time gate would take the decision away from segments that rarely skip: fewer skips to get wrong)."""
    if (name, gate) not in _PACKS:
        cs = workloads.build_constraints(_raw(name))
        prev = os.environ.get("RAYEN_PAIR_SCREEN_GATE")
        if not gate:
            os.environ["RAYEN_PAIR_SCREEN_GATE"] = "0"
        try:
            layer = ConstraintModule(cs, method="RAYEN", create_map=False).to("cuda")
            dp, _ = layer.device_pack(torch.device("cuda", torch.cuda.current_device()))
        finally:
            if not gate:
                if prev is None:
                    del os.environ["RAYEN_PAIR_SCREEN_GATE"]
                else:
                    os.environ["RAYEN_PAIR_SCREEN_GATE"] = prev
        assert dp.info().mfma_f32 == 3, "the f16-pair family serves this pack"
        _PACKS[(name, gate)] = (cs, layer, dp)
    return _PACKS[(name, gate)]


@pytest.fixture
def lib():
    lib = _lib.load()
    prev_schedule, prev_screen = lib.rayen_pair_schedule(3), lib.rayen_pair_screen(-1)
    yield lib
    lib.rayen_pair_screen_counters(None)
    lib.rayen_pair_screen(prev_screen)
    lib.rayen_pair_schedule(prev_schedule)


def _both(lib, dp, v, want_active):
    out = []
    for mode in (0, 1):
        lib.rayen_pair_screen(mode)
        assert lib.rayen_pair_screen(-1) == mode
        dp.nan_flag.zero_()
        y, kappa, active = ops.project_raw(v, dp, want_active=want_active)
        assert lib.rayen_last_forward_kernel() == _lib.KERNEL_PAIR_WL
        out.append((y, kappa, active, int(dp.nan_flag.item())))
    dp.nan_flag.zero_()
    return out


def _same(a, b):
    # (bit patterns: NaN rows compare equal to themselves)
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _rows(B, n, seed):
    v = torch.empty(B, n, device="cuda").uniform_(-1.5, 1.5, generator=torch.Generator(device="cuda").manual_seed(seed))
    if B >= 33:      # (one of each inside the first two groups, next to ordinary rows; again in the last, ragged group)
        v[3] *= 1e-20
        v[7] *= 1e20
        v[11] = 0.0
        v[13, 5] = float("nan")
        v[17, 0] = float("inf")
        v[32] *= 1e-20
        v[B - 1] *= 1e20
    if B >= 1000:
        v[B - 3] = 0.0
        v[B - 5, 1] = float("-inf")
        v[B - 40, 2] = float("nan")
        v[500:532] *= 1e-20          # a whole group of tiny rows, a whole group of huge ones
        v[532:564] *= 1e20
    return v


@pytest.mark.parametrize("want_active", [False, True])
@pytest.mark.parametrize("B", [1, 33, 1000, 4096 + 7])
@pytest.mark.parametrize("name", ["c3", "n64_many_aux", "n32", "n36", "c3_gated"])
def test_screening_changes_no_bit(name, B, want_active, lib):
    cs, layer, dp = _pack("c3", gate=True) if name == "c3_gated" else _pack(name)      # (c3_gated: the pack as a user gets it)
    v = _rows(B, cs.n, 1000 * B + len(name))
    (y0, k0, a0, f0), (y1, k1, a1, f1) = _both(lib, dp, v, want_active)
    assert _same(y0, y1) and _same(k0, k1)
    assert f0 == f1 == (1 if B >= 33 else 0)
    if want_active:
        assert torch.equal(a0, a1)


@pytest.mark.parametrize("B", [33, 4096 + 7])
def test_a_cone_that_is_active_on_half_the_rows(B, lib):
    """Groups that skip the cone next to groups that walk it, and lanes on the cone next to lanes far below it."""
    cs, layer, dp = _pack("c3_cone_half_active")
    v = _rows(B, cs.n, 77 + B)
    (y0, k0, a0, _), (y1, k1, a1, _) = _both(lib, dp, v, True)
    assert _same(y0, y1) and _same(k0, k1) and torch.equal(a0, a1)
    cones = [i for i, s in enumerate(dp.consts.segments) if s.type == _lib.SEG_SOC]
    # the same rows sorted by whether the cone set kappa: whole groups far below it, whole groups on it, one mixed group
    order = torch.argsort((a0[:, 0] == cones[0]).int(), stable=True)
    vs = v[order].contiguous()
    counts = torch.zeros(64, dtype=torch.int32, device="cuda")
    lib.rayen_pair_screen_counters(ctypes.c_void_p(counts.data_ptr()))
    (ys0, ks0, as0, _), (ys1, ks1, as1, _) = _both(lib, dp, vs, True)
    torch.cuda.synchronize()
    lib.rayen_pair_screen_counters(None)
    assert _same(ys0, ys1) and _same(ks0, ks1) and torch.equal(as0, as1)
    assert _same(ys1, y1[order]) and _same(ks1, k1[order]) and torch.equal(as1, a1[order])      # (rows are independent)
    groups = (B + 31) // 32
    skipped = int(counts[cones[0]])
    print(f"\n  B = {B}: sorted rows, the scaled cone was skipped for {skipped} of {groups} groups")
    assert skipped < groups
    if B > 4096:
        assert 0 < int(counts.sum()) < groups * len(dp.consts.segments)
    ok = torch.isfinite(k1) & (k1 > 0)
    share = float((a1[ok, 0] == cones[0]).float().mean())
    print(f"\n  B = {B}: the scaled cone is active on {share:.3f} of the rows")
    assert 0.25 <= share <= 0.75, share


def test_most_groups_of_config_3_skip_their_cones(lib):
    """The counter: per segment, the 32-sample groups for which it was skipped.  At c3 seed 7, U(-1.5, 1.5), the fp64 evaluator
    with the same bound skips 0.83 / 0.93 of the groups for the two cones; at least half each must be seen here -- a condition
    that keeps the equalities above from being vacuous, not a tuning target."""
    cs, layer, dp = _pack("c3", gate=True)
    B = 4096
    v = torch.empty(B, cs.n, device="cuda").uniform_(-1.5, 1.5, generator=torch.Generator(device="cuda").manual_seed(1000))
    counts = torch.zeros(64, dtype=torch.int32, device="cuda")
    lib.rayen_pair_screen(1)
    lib.rayen_pair_screen_counters(ctypes.c_void_p(counts.data_ptr()))
    ops.project_raw(v, dp, want_active=False)
    assert lib.rayen_last_forward_kernel() == _lib.KERNEL_PAIR_WL
    torch.cuda.synchronize()
    lib.rayen_pair_screen_counters(None)
    once = counts.cpu().clone()
    ops.project_raw(v, dp, want_active=False)          # disarmed: nothing is counted
    torch.cuda.synchronize()
    assert torch.equal(counts.cpu(), once)
    lib.rayen_pair_screen(0)                           # armed but screening off: nothing to count
    lib.rayen_pair_screen_counters(ctypes.c_void_p(counts.data_ptr()))
    ops.project_raw(v, dp, want_active=False)
    torch.cuda.synchronize()
    lib.rayen_pair_screen_counters(None)
    assert torch.equal(counts.cpu(), once)
    groups = B // 32
    cones = [i for i, s in enumerate(dp.consts.segments) if s.type == _lib.SEG_SOC]
    shares = {i: int(once[i]) / groups for i in range(len(dp.consts.segments))}
    print(f"\n  skipped share of {groups} groups per segment: {shares}")
    assert len(cones) == 2
    for i in cones:
        assert 0.5 <= shares[i] <= 1.0, shares
    assert all(int(once[i]) == 0 for i in range(len(dp.consts.segments), 64))
