"""The sweep's reference (tests/dc3_reference.py) checked on the host: against the real reference's recorded outputs
(fixtures under tests/golden/dc3), and every case, input and stop position of tests/test_gpu_dc3_sweep.py for soundness --
finite, stop decided by a margin of at least 0.5 %, the same count in fp32 and fp64, kink rows within the cap."""
import numpy as np
import pytest
import torch

import dc3_cases
import dc3_reference as ref
from rayen_amd import dc3

KiB = 1024


@pytest.mark.parametrize("mode", dc3_cases.MODES)
@pytest.mark.parametrize("name", dc3_cases.NAMES)
def test_reference_reproduces_the_fixtures(name, mode):
    layer, z = dc3_cases.layer_for(name, torch.float64)
    _, args, _ = dc3_cases.load(name)
    arrays = dc3.pack_arrays(layer)
    limit = args["max_steps_training" if mode == "train" else "max_steps_testing"]
    q = z["q"][:, :, 0].astype(np.float64)
    out = ref.forward_ref(arrays, q, args["lr"], args["momentum"], args["eps_converge"], limit)
    assert out.steps == int(z[f"steps64_{mode}"])
    assert out.v.shape == (out.steps + 1,) and out.res.shape[:2] == (out.steps + 1, q.shape[0])
    assert dc3_cases.row_err(out.y, z[f"y64_{mode}"]).max() <= 1e-11
    grad = ref.backward_ref(arrays, q, z["w"], args["lr"], args["momentum"], out.steps)
    assert dc3_cases.row_err(grad, z[f"gq64_{mode}"]).max() <= 1e-11


def test_cases_cover_every_instance_and_every_listed_value():
    cases = ref.CASES
    assert len({c.name for c in cases}) == len(cases)
    # every (dtype, NP) the kernels instantiate, with padding lanes and without
    for NP in (4, 8, 16, 32, 64):
        mine = [c for c in cases if ref.pad_n(c.n) == NP]
        assert any(c.n < NP for c in mine) and any(c.n == NP for c in mine), NP
        for dtype in (torch.float32, torch.float64):
            assert all(ref.served(c, dtype) == (dtype == torch.float32 or NP <= 32) for c in mine)
    assert {c.n for c in cases} >= {1, 4, 5, 8, 9, 16, 17, 32, 33, 64}
    assert {c.m for c in cases} >= {0, 1, 5, 6, 48, 128}
    assert {c.nq for c in cases} >= {0, 1, 3, 4}
    assert {c.no for c in cases} >= {0, 1, 3, 5}
    assert any(c.m % 4 and c.nq > 0 for c in cases)              # off_q depends on round4(m)
    assert any(c.no % 4 and c.no > 0 for c in cases)
    assert any(c.m == 0 and c.nq > 0 for c in cases)
    assert any(c.nq == 0 and c.m > 0 for c in cases)
    assert any(c.no > 0 and c.nq >= 2 for c in cases)
    assert any((c.n, c.m, c.nq) == (64, 128, 4) for c in cases)
    assert [ref.pad_n(ref.CASE[name].n) for name in ref.POSITION_CASES] == [4, 8, 16, 32, 64]
    assert {p for p in ref.POSITIONS if p[1] is not None} >= {
        (1, 1), (32, 32), (33, 33), (33, 32), (100, 1), (100, 2), (100, 31), (100, 32), (100, 33), (100, 64), (100, 65),
        (100, 96), (100, 97)}
    assert {p[0] for p in ref.POSITIONS if p[1] is None} == {32, 33, 100}
    assert ref.EQUALITIES_ONLY.m == 0 and ref.EQUALITIES_ONLY.nq == 0 and ref.EQUALITIES_ONLY.no > 0


def test_lds_cases_land_in_their_byte_ranges():
    L = ref.LDS_CASE
    assert 48 * KiB < ref.lds_bytes(L["lds_above_48k"], 4) < 64 * KiB
    assert ref.LDS_LIMIT == 160 * KiB - 256
    assert ref.LDS_LIMIT - KiB <= ref.lds_bytes(L["lds_at_the_limit"], 4) <= ref.LDS_LIMIT
    assert ref.LDS_LIMIT < ref.lds_bytes(L["lds_just_over"], 4) <= ref.LDS_LIMIT + KiB
    only32 = L["lds_fp32_only"]
    assert only32.n <= 32 and ref.lds_bytes(only32, 4) <= ref.LDS_LIMIT < ref.lds_bytes(only32, 8)
    assert ref.served(only32, torch.float32) and not ref.served(only32, torch.float64)
    assert not ref.served(L["lds_just_over"], torch.float32)
    assert all(ref.lds_bytes(c, 8) <= 48 * KiB for c in ref.CASES if c.n <= 16)      # (small images stay small)


def test_packs_are_what_the_issue_describes():
    for case in ref.CASES + ref.LDS_CASES + [ref.EQUALITIES_ONLY]:
        a = ref.make_pack(case)
        n, k = case.n, case.n + case.no
        assert a["A1e"].shape == (case.m, n) and a["Pe"].shape == (case.nq, n, n) and a["C"].shape == (case.no, n)
        assert a["n"] == n and a["k"] == k and a["partial"].dtype == np.int32 and a["other"].dtype == np.int32
        assert sorted(list(a["partial"]) + list(a["other"])) == list(range(k))
        if case.no and n > 1:
            assert list(a["partial"]) != sorted(a["partial"]) or max(a["partial"]) > n - 1       # interleaved
        assert np.all(a["b1e"] > 0) and np.all(a["re"] < 0)
        if case.m:
            norms = np.linalg.norm(a["A1e"], axis=1)
            assert norms.min() > 0.75 and norms.max() < 1.25
        for P in a["Pe"]:
            assert np.linalg.eigvalsh(0.5 * (P + P.T)).min() > -0.7
            assert (np.abs(P - P.T).max() > 1e-3) == (case.no > 0)
        for key in ("A1e", "b1e", "Pe", "qe", "re", "C", "c0"):
            assert np.array_equal(a[key], a[key].astype(np.float32).astype(np.float64)) and a[key].flags.c_contiguous


def _sweep_calls():
    out = []
    for case in ref.CASES:
        for B in ref.SWEEP_BATCHES:
            out += [(case.name, B, *ref.TRAIN_CALL), (case.name, B, *ref.EVAL_CALL)]
    for name in ref.POSITION_CASES:
        out += [(name, ref.POSITION_BATCH, *position) for position in ref.POSITIONS]
    for case in ref.LDS_CASES:
        if ref.served(case, torch.float32):
            out += [(case.name, 257, *ref.TRAIN_CALL), (case.name, 257, *ref.EVAL_CALL)]
    return sorted(set(out), key=str)


def _sound(call, expect_steps, B):
    assert np.isfinite(call.y64).all() and np.isfinite(call.gq64).all() and np.isfinite(call.v).all()
    assert call.steps == expect_steps
    assert call.steps32 == call.steps
    assert ref.stop_margin(call.v, call.eps, call.steps, call.max_steps)
    assert int(call.kinks.sum()) <= ref.kink_cap(B), (int(call.kinks.sum()), B)
    assert call.gap_y < 1e-5 and call.gap_g < 1e-3             # (the two host runs are runs of the same thing)


@pytest.mark.parametrize("name,B,max_steps,t_star", _sweep_calls())
def test_every_call_of_the_sweep_is_sound(name, B, max_steps, t_star):
    call = ref.call_for(name, B, max_steps, t_star)            # (eps_for asserts the 1 % fall at t_star)
    _sound(call, max_steps if t_star is None else t_star, B)


@pytest.mark.parametrize("case", ref.CASES + ref.LDS_CASES, ids=lambda c: c.name)
def test_every_case_stays_finite_over_100_steps_and_uses_its_constraints(case):
    arrays = ref.make_pack(case)
    for B in (1, 257):
        q, _ = ref.make_inputs(case, B)
        out = ref.forward_ref(arrays, q, case.lr, ref.MOMENTUM, 0.0, 100)
        assert out.steps == 100 and np.isfinite(out.y).all() and np.isfinite(out.res).all()
        assert np.all(out.v[1:] > 0)
    # both kinds of constraint are violated by a good share of the rows (a kernel that dropped one would be seen)
    first = out.res[0]
    if case.m:
        assert (first[:, :case.m] > 0).any(axis=1).mean() >= 0.1
    if case.nq:
        assert (first[:, case.m:] > 0).any(axis=1).mean() >= 0.5


@pytest.mark.parametrize("B", ref.OUTLIER_BATCHES)
def test_the_outlier_calls_are_sound(B):
    far, near = ref.outlier_calls(B)
    _sound(far, ref.OUTLIER_CALL[1], B)
    _sound(near, 1, B)
    assert np.all(near.v == 0)                                 # every row of the batch starts inside
    # row B - 1 alone decides: without it the same rows stop at once
    alone = ref.forward_ref(far.arrays, far.q[B - 1:], far.lr, far.momentum, far.eps, far.max_steps)
    assert alone.steps == far.steps and np.allclose(alone.v, far.v, rtol=1e-10, atol=0)
    # a row at the origin (where a kernel's inactive lanes sit) is outside by far more than eps, at every step
    origin = ref.forward_ref(far.arrays, np.zeros((1, far.q.shape[1])), far.lr, far.momentum, 0.0, far.max_steps)
    assert np.all(origin.v[1:] > 2 * far.eps)


def test_a_set_of_equalities_only_runs_to_the_limit():
    case = ref.EQUALITIES_ONLY
    arrays = ref.make_pack(case)
    q, gy = ref.make_inputs(case, 65)
    out = ref.forward_ref(arrays, q, case.lr, ref.MOMENTUM, 1e-3, 12)
    assert out.steps == 12 and np.all(out.v == 0)
    assert np.array_equal(out.y[:, arrays["partial"]], q)
    assert np.allclose(out.y[:, arrays["other"]], arrays["c0"] + q @ arrays["C"].T, rtol=0, atol=1e-14)


def test_eps_for_refuses_a_stop_within_rounding():
    v = np.array([1.0, 0.5, 0.25, 0.249, 0.1])
    assert ref.eps_for(v, 2) == pytest.approx(np.sqrt(0.25 * 0.5))
    assert ref.eps_for(v, 1) == pytest.approx(np.sqrt(0.5))
    assert 0.1 < ref.eps_for(v, 4) < 0.249
    with pytest.raises(AssertionError):
        ref.eps_for(v, 3)


def test_kink_rows_marks_near_zero_and_flipped_residuals():
    r64 = np.array([[[0.5, -0.5], [1e-7, 0.3], [1e-9, 0.2], [0.3, -0.4]]])          # [1 step, 4 rows, 2 residuals]
    r32 = r64 + np.array([[[1e-7, 1e-7], [5e-8, 0.0], [-2e-9, 0.0], [0.0, 0.0]]])
    assert ref.kink_rows(r64, r32).tolist() == [False, True, True, False]
