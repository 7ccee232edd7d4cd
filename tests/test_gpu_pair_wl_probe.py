"""The leading-product probe of the W-in-LDS schedule (rayen_amd/csrc/rayen_mfma_pair_wl.hip, round 8): in front of a
quadratic / cone the spectral test did not rule out, the walk multiplies only the leading f16 pieces a1 b1 of the segment (a
third of its MFMAs), bounds the sum of squares the full walk would reach, and skips the segment when that bound through the
segment's own closer is below the running maximum of every live sample; this schedule also walks its quadratics / cones in the
order of how often each sets kappa.  A skip and the order must change NOTHING: y, kappa, the arg-max record and the NaN flag
with probe and spectral test (mode 1) equal those of the spectral test alone (mode 2) and of no screening (mode 0) bit for bit
-- on every set shape the schedule serves, gated and ungated packs, ragged batches, rows of every magnitude, zero, NaN and
infinite rows, sets of identical segments (every candidate equals the running maximum: nothing may be skipped), and rows on
which a quadratic's candidate is within 2^-12 .. 2^-6 of another segment's.  So that the equalities are not vacuous, the
counters must report that most groups of config 3 do skip three of its four quadratics.  Needs an MI355X."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import rayen_oracle as oracle
from rayen_amd import _lib, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

pytestmark = pytest.mark.gpu


def _identical(kind):
    """Five times the same tight quadratic / three times the same tight cone, next to linear rows far outside them."""
    raw = workloads.random_lin_quad_soc(k=64, m=32, n_quad=1 if kind == "quad" else 0, n_soc=0 if kind == "quad" else 1, seed=31)
    raw["b1"] = raw["b1"] * 1e3
    if kind == "quad":
        for key in ("P", "q", "r"):
            raw[key] = [raw[key][0].copy() for _ in range(5)]
    else:
        for key in ("M", "s", "c", "d"):
            raw[key] = [raw[key][0].copy() for _ in range(3)]
    return raw


def _raw(name):
    if name == "c3":
        return workloads.make_raw("c3", seed=7)
    if name == "c3_seed0":
        return workloads.make_raw("c3", seed=0)
    return {"n64_many_aux": lambda: workloads.random_lin_quad_soc(k=64, m=32, n_quad=5, n_soc=3, seed=25),
            "n32": lambda: workloads.random_lin_quad_soc(k=32, m=300, n_quad=3, n_soc=2, seed=17),
            "n36": lambda: workloads.random_lin_quad_soc(k=36, m=100, n_quad=2, n_soc=1, seed=23),
            "same_quads": lambda: _identical("quad"),
            "same_cones": lambda: _identical("cone")}[name]()


_PACKS = {}


def _make(raw, gate):
    cs = workloads.build_constraints(raw)
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
    return cs, layer, dp


def _pack(name, gate):
    """gate=False: created with RAYEN_PAIR_SCREEN_GATE=0 -- every qualifying segment is decided AND probed (the failing probe's
    path runs); gate=True: the pack as a user gets it."""
    if (name, gate) not in _PACKS:
        _PACKS[(name, gate)] = _make(_raw(name), gate)
    return _PACKS[(name, gate)]


@pytest.fixture
def lib():
    lib = _lib.load()
    prev_schedule, prev_screen = lib.rayen_pair_schedule(3), lib.rayen_pair_screen(-1)
    yield lib
    lib.rayen_pair_screen_counters(None)
    lib.rayen_pair_screen(prev_screen)
    lib.rayen_pair_schedule(prev_schedule)


def _run(lib, dp, v, want_active, mode, counts=None):
    lib.rayen_pair_screen(mode)
    assert lib.rayen_pair_screen(-1) == mode
    dp.nan_flag.zero_()
    if counts is not None:
        counts.zero_()
        lib.rayen_pair_screen_counters(ctypes.c_void_p(counts.data_ptr()))
    y, kappa, active = ops.project_raw(v, dp, want_active=want_active)
    assert lib.rayen_last_forward_kernel() == _lib.KERNEL_PAIR_WL
    torch.cuda.synchronize()
    if counts is not None:
        lib.rayen_pair_screen_counters(None)
    flag = int(dp.nan_flag.item())
    dp.nan_flag.zero_()
    return y, kappa, active, flag


def _same(a, b):
    # (bit patterns: NaN rows compare equal to themselves)
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _rows(B, n, seed):
    """The rows of test_gpu_pair_wl_screen.py::_rows."""
    v = torch.empty(B, n, device="cuda").uniform_(-1.5, 1.5, generator=torch.Generator(device="cuda").manual_seed(seed))
    if B >= 33:
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
        v[500:532] *= 1e-20
        v[532:564] *= 1e20
    return v


@pytest.mark.parametrize("want_active", [False, True])
@pytest.mark.parametrize("B", [1, 33, 1000, 4096 + 7])
@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("name", ["c3", "c3_seed0", "n64_many_aux", "n32", "n36", "same_quads", "same_cones"])
def test_the_probe_changes_no_bit(name, gate, B, want_active, lib):
    cs, layer, dp = _pack(name, gate)
    v = _rows(B, cs.n, 1000 * B + len(name))
    counts = torch.zeros(64, dtype=torch.int32, device="cuda")
    y0, k0, a0, f0 = _run(lib, dp, v, want_active, 0)
    y2, k2, a2, f2 = _run(lib, dp, v, want_active, 2)
    y1, k1, a1, f1 = _run(lib, dp, v, want_active, 1, counts)
    assert _same(y0, y1) and _same(k0, k1) and _same(y2, y1) and _same(k2, k1)
    assert f0 == f1 == f2 == (1 if B >= 33 else 0)
    if want_active:
        assert torch.equal(a0, a1) and torch.equal(a2, a1)
    if name.startswith("same_"):
        assert int(counts.sum()) == 0, counts.tolist()      # (every candidate equals the running maximum)


def _near_tie_raw(j, bits):
    """Config 3 (seed 7) with quadratic j rescaled so that, along the top eigenvector u of its Delta, its candidate is
    1 - 2^-bits of the largest other candidate (fp64 oracle).  P -> a^2 P, q -> a q multiplies the candidate by a."""
    raw = workloads.make_raw("c3", seed=7)
    cs = workloads.build_constraints(raw)
    csd = {key: getattr(cs, key) for key in ("A_p", "b_p", "NA_E", "yp", "z0", "y0")}
    csd.update(P=raw["P"], q=raw["q"], r=raw["r"], M=raw["M"], s=raw["s"], c=raw["c"], d=raw["d"], F=raw["F"])
    buf = oracle.precompute(csd, torch.float64)
    lam, vec = torch.linalg.eigh(buf["all_delta"][j])
    u = vec[:, -1]
    cand = oracle.compute_kappa(buf, u.reshape(1, -1, 1), terms=True)[0]
    m = buf["D"].shape[0]
    own = float(cand[m + j])
    other = float(torch.cat((cand[:m + j], cand[m + j + 1:])).max())
    assert own > 0 and other > 0
    a = other / own * (1.0 - 2.0 ** -bits)
    raw["P"][j] = raw["P"][j] * a * a
    raw["q"][j] = raw["q"][j] * a
    return raw, u


@pytest.mark.parametrize("bits", [12, 9, 6])
def test_near_ties(bits, lib):
    """Groups of rows around the direction on which quadratic 1's candidate is within 2^-bits of the largest other one: the
    outputs with the probe equal those without it, and a group in which the fp64 oracle has the quadratic at the maximum
    for some row was not skipped."""
    j = 1
    raw, u = _near_tie_raw(j, bits)
    cs, layer, dp = _make(raw, gate=False)
    csd = {key: getattr(cs, key) for key in ("A_p", "b_p", "NA_E", "yp", "z0", "y0")}
    csd.update(P=raw["P"], q=raw["q"], r=raw["r"], M=raw["M"], s=raw["s"], c=raw["c"], d=raw["d"], F=raw["F"])
    buf = oracle.precompute(csd, torch.float64)
    gen = torch.Generator().manual_seed(100 + bits)
    n_groups = 6
    rows = []
    for g in range(n_groups):
        noise = torch.randn(32, cs.n, generator=gen, dtype=torch.float64) * (2.0 ** -(bits + 2)) * (g / 2.0)
        rows.append((u.reshape(1, -1) + noise) * (1.0 + g))      # (group 0: 32 times the direction itself)
    vd = torch.cat(rows, dim=0)
    v = vd.to(torch.float32).to("cuda")
    cand = oracle.compute_kappa(buf, torch.nn.functional.normalize(v.cpu().double(), dim=1).unsqueeze(2), terms=True)
    m = buf["D"].shape[0]
    quad_is_max = (cand.argmax(dim=1) == m + j).reshape(n_groups, 32).any(dim=1)
    quads = [i for i, s in enumerate(dp.consts.segments) if s.type in (_lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC)]
    assert len(quads) == 4
    counts = torch.zeros(64, dtype=torch.int32, device="cuda")
    y0, k0, a0, _ = _run(lib, dp, v, True, 0)
    y1, k1, a1, _ = _run(lib, dp, v, True, 1)
    assert _same(y0, y1) and _same(k0, k1) and torch.equal(a0, a1)
    skipped = []
    for g in range(n_groups):
        vg = v[32 * g:32 * g + 32].contiguous()
        yg, kg, ag, _ = _run(lib, dp, vg, True, 1, counts)
        assert _same(yg, y0[32 * g:32 * g + 32]) and _same(kg, k0[32 * g:32 * g + 32]) and torch.equal(ag, a0[32 * g:32 * g + 32])
        skipped.append(int(counts[quads[j]]))
        if bool(quad_is_max[g]):
            assert skipped[-1] == 0, (g, skipped)
    gap = (cand[:, m + j] / torch.cat((cand[:, :m + j], cand[:, m + j + 1:]), dim=1).max(dim=1).values - 1.0).reshape(n_groups, 32)
    print(f"\n  2^-{bits}: per group, quadratic {j} at the maximum (fp64) {quad_is_max.tolist()}, skipped {skipped}, "
          f"relative gap to the largest other candidate {[f'{float(x.min()):+.2e}..{float(x.max()):+.2e}' for x in gap]}")


def test_most_groups_of_config_3_skip_three_quadratics(lib):
    """c3 seed 7, the pack as a user gets it, U(-1.5, 1.5): the fp64 evaluator with the same margin has q1, q2 and q3 below the
    running maximum in 0.99 of the groups; at least half each must be seen here -- a condition that keeps the equalities above
    from being vacuous, not a tuning target."""
    cs, layer, dp = _pack("c3", True)
    B = 4096
    v = torch.empty(B, cs.n, device="cuda").uniform_(-1.5, 1.5, generator=torch.Generator(device="cuda").manual_seed(1000))
    counts = torch.zeros(64, dtype=torch.int32, device="cuda")
    _run(lib, dp, v, False, 1, counts)
    both = counts.cpu().clone()
    _run(lib, dp, v, False, 2, counts)
    bound_only = counts.cpu().clone()
    groups = B // 32
    quads = [i for i, s in enumerate(dp.consts.segments) if s.type in (_lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC)]
    shares = {i: int(both[i]) / groups for i in range(len(dp.consts.segments))}
    print(f"\n  skipped share of {groups} groups per segment, probe and spectral test: {shares}")
    print(f"  spectral test alone: { {i: int(bound_only[i]) / groups for i in range(len(dp.consts.segments))} }")
    assert len(quads) == 4
    for i in quads[1:]:
        assert 0.5 <= shares[i] <= 1.0, shares
    assert all(int(both[i]) <= groups for i in range(64))
    assert all(int(both[i]) == 0 for i in range(len(dp.consts.segments), 64))
