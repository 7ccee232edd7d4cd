"""Sweep of the DC3 kernels (rayen_amd/csrc/rayen_dc3.hip) on the MI355X against the fp64 host reference of
tests/dc3_reference.py: every instance ``dc3_{forward,backward}_kernel<float, 4..64>`` / ``<double, 4..32>``, every stop
position relative to the 32-step launches (a chunk's end, its first step, all four chunks of 100 steps and both ping-pong
parities as replay source, limits that are no multiple of 32), LDS images above the 48 KiB opt-in and at the limit, the
paddings of the image, and the deciding row in the last, partial wave.  Synthetic packs go straight through
``ops.Dc3Pack`` / ``ops.dc3_forward_raw`` / ``ops.dc3_backward_raw``.

Bars (those of tests/test_gpu_dc3.py): ``dc3_cases.row_err`` against the fp64 reference at most 1e-11 in fp64, and in fp32
at most max(4 x the host's own fp32-versus-fp64 gap of the same call, 1e-5), ``y`` and ``grad_q`` separately.  The forward
is asserted on every row; the backward on every row outside ``dc3_reference.kink_rows`` (a residual within rounding of
zero: ``diag[r > 0]`` is discontinuous there), whose number is held to max(2, 2 % of the batch) -- a condition on the
inputs that tests/test_dc3_reference_host.py has already shown on the host.  ``steps`` must equal the host's count; eps sits
at least 0.5 % away from the violations on either side of the stop, so the decision is never within rounding."""
import warnings

import numpy as np
import pytest
import torch

import dc3_cases
import dc3_reference as ref
from rayen_amd import _lib, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = {torch.float32: 1e-5, torch.float64: 1e-11}
DTYPES = [torch.float32, torch.float64]
TAG = {torch.float32: "fp32", torch.float64: "fp64"}

_packs = {}


def _pack(key, arrays):
    if key not in _packs:
        _packs[key] = ops.Dc3Pack(arrays, 0)
    return _packs[key]


def _dev(x, dtype):
    return torch.tensor(x).to(dtype).to(DEV)


def _check(label, pack, call, dtype, rows=None):
    """One forward + backward of ``call`` at ``dtype`` against its host reference (``rows``: the rows compared, all by
    default).  Returns (y, steps, grad_q) as the kernels left them."""
    B, n, k = call.q.shape[0], pack.n, pack.k
    rows = np.ones(B, dtype=bool) if rows is None else rows
    # two more columns than n, of junk: the kernels read n columns and grad_q is zero beyond them
    q = torch.full((B, n + 2), float("nan"), dtype=dtype, device=DEV)
    q[:, :n] = _dev(call.q, dtype)
    gy = _dev(call.gy, dtype)
    y, steps = ops.dc3_forward_raw(q, pack, call.lr, call.momentum, call.eps, call.max_steps)
    grad = ops.dc3_backward_raw(q, steps, gy, pack, call.lr, call.momentum, call.max_steps)
    assert y.shape == (B, k) and y.dtype == dtype and steps.shape == (1,) and steps.dtype == torch.int32
    assert grad.shape == q.shape and grad.dtype == dtype
    taken = int(steps.item())
    yh, gh = y.cpu().numpy(), grad.cpu().numpy()
    keep = rows & ~call.kinks
    gap_y, gap_g = ref.gaps(call, rows, keep) if dtype == torch.float32 else (0.0, 0.0)
    bar_y, bar_g = max(4.0 * gap_y, FLOOR[dtype]), max(4.0 * gap_g, FLOOR[dtype])
    err_y = dc3_cases.row_err(yh[rows], call.y64[rows]).max()
    err_g = dc3_cases.row_err(gh[keep][:, :n], call.gq64[keep]).max() if keep.any() else 0.0
    print(f"{label} {TAG[dtype]} B={B} limit={call.max_steps}: steps {taken} (host {call.steps})  y err {err_y:.3e} bar "
          f"{bar_y:.3e} ratio {err_y / bar_y:.3f}  grad err {err_g:.3e} bar {bar_g:.3e} ratio {err_g / bar_g:.3f}  "
          f"kinks {int(call.kinks.sum())}")
    assert taken == call.steps
    assert np.isfinite(yh[rows]).all() and np.isfinite(gh[rows]).all()
    assert np.all(gh[:, n:] == 0)
    assert int(call.kinks[rows].sum()) <= ref.kink_cap(B)
    assert err_y <= bar_y
    assert err_g <= bar_g
    return y, steps, grad


def _case_check(case, dtype, B, max_steps, t_star):
    call = ref.call_for(case.name, B, max_steps, t_star)
    return _check(f"{case.name} t*={t_star}", _pack(case.name, call.arrays), call, dtype)


def _instances(cases):
    return [pytest.param(c, dt, id=f"{c.name}-{TAG[dt]}") for c in cases for dt in DTYPES if ref.served(c, dt)]


@pytest.mark.parametrize("case,dtype", _instances(ref.CASES))
def test_every_instance(case, dtype):
    for B in ref.SWEEP_BATCHES:
        _case_check(case, dtype, B, *ref.TRAIN_CALL)
        _case_check(case, dtype, B, *ref.EVAL_CALL)


@pytest.mark.parametrize("position", ref.POSITIONS, ids=lambda p: f"limit{p[0]}-stop{p[1]}")
@pytest.mark.parametrize("case,dtype", _instances([ref.CASE[name] for name in ref.POSITION_CASES]))
def test_stop_positions(case, dtype, position):
    max_steps, t_star = position
    _, steps, _ = _case_check(case, dtype, ref.POSITION_BATCH, max_steps, t_star)
    assert int(steps.item()) == (max_steps if t_star is None else t_star)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("B", ref.OUTLIER_BATCHES)
def test_deciding_row_in_the_last_partial_wave(B, dtype):
    far, near = ref.outlier_calls(B)
    pack = _pack("outlier", far.arrays)
    _, steps_far, _ = _check(f"outlier row {B - 1}", pack, far, dtype)
    _, steps_near, _ = _check("outlier row replaced", pack, near, dtype)
    # the inactive lanes of the last wave sit at the origin, outside this set: they must not hold the stop back
    assert int(steps_near.item()) == near.steps == 1 < int(steps_far.item()) == ref.OUTLIER_CALL[1]


def _raw_calls_refused(case, dtype):
    arrays = ref.make_pack(case)
    pack = _pack(case.name, arrays)
    q, gy = (_dev(x, dtype) for x in ref.make_inputs(case, 65))
    with pytest.raises(_lib.RayenError) as info:
        ops.dc3_forward_raw(q, pack, case.lr, ref.MOMENTUM, 1e-3, 10)
    assert info.value.code == _lib.E_UNSUPPORTED
    steps = torch.tensor([3], dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.RayenError) as info:
        ops.dc3_backward_raw(q, steps, gy, pack, case.lr, ref.MOMENTUM, 10)
    assert info.value.code == _lib.E_UNSUPPORTED


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("name", [c.name for c in ref.LDS_CASES])
def test_large_images(name, dtype):
    case = ref.LDS_CASE[name]
    if ref.served(case, dtype):
        _case_check(case, dtype, 257, *ref.TRAIN_CALL)
        _case_check(case, dtype, 257, *ref.EVAL_CALL)
    else:
        assert (name, dtype) in (("lds_just_over", torch.float32), ("lds_just_over", torch.float64),
                                 ("lds_fp32_only", torch.float64), ("lds_at_the_limit", torch.float64))      # (n = 64)
        _raw_calls_refused(case, dtype)


def test_fp64_beyond_32_variables():
    for name in ("np64_n33_nearly_unconstrained", "np64_n64_five_equalities"):
        case = ref.CASE[name]
        _raw_calls_refused(case, torch.float64)
        _case_check(case, torch.float32, 65, *ref.TRAIN_CALL)
    beyond = ref.Case("n65_beyond_the_registers", 65, 1, 0, 0, 1e-2, 0.5)
    for dtype in DTYPES:
        _raw_calls_refused(beyond, dtype)


@pytest.mark.eager_detour
def test_a_module_beyond_32_variables_detours_in_fp64_only(monkeypatch):
    raw = workloads.random_lin_quad_soc(k=40, m=30, n_quad=1, n_soc=0, seed=6)
    args = dict(lr=1e-4, momentum=0.5, eps_converge=1e-3, max_steps_training=5, max_steps_testing=5)
    layer = ConstraintModule(workloads.build_constraints(raw), method="DC3", create_map=False, args_DC3=args).to(DEV)
    q = torch.rand(64, 40, 1, device=DEV) - 0.5
    monkeypatch.setenv("RAYEN_STRICT_HIP", "1")
    with pytest.raises(_lib.RayenError):
        layer(q.double())
    monkeypatch.delenv("RAYEN_STRICT_HIP")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        y = layer(q.double())
        layer(q.double())
    said = [w for w in seen if issubclass(w.category, RuntimeWarning) and "no HIP kernel serves this DC3" in str(w.message)]
    assert len(said) == 1 and layer._hip_unsupported
    assert y.dtype == torch.float64 and torch.equal(y, layer._dc3_reference(q.double()))
    # the refusal is per dtype: fp32 input still reaches the kernel
    calls = []
    real = ops.dc3_forward_raw
    monkeypatch.setattr(ops, "dc3_forward_raw", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(layer, "_dc3_reference", lambda *a, **k: (_ for _ in ()).throw(AssertionError("eager detour")))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y32 = layer(q)
    assert calls and y32.dtype == torch.float32
    assert dc3_cases.row_err(y32.cpu()[:, :, 0], y.cpu()[:, :, 0]).max() <= 1e-5


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_layouts(dtype):
    case = ref.CASE["np8_n5_ragged_everything"]
    call = ref.call_for(case.name, 257, *ref.EVAL_CALL)
    pack = _pack(case.name, call.arrays)
    n, k, B = case.n, case.n + case.no, 257
    run = lambda q, gy: _run(pack, call, q, gy)                # noqa: E731
    q, gy = _dev(call.q, dtype), _dev(call.gy, dtype)
    y0, s0, g0 = run(q, gy)
    assert int(s0.item()) == call.steps and g0.shape == (B, n)
    y1, s1, g1 = run(q, gy)                                    # the atomic max is order-free: the same bits again
    assert torch.equal(y1, y0) and torch.equal(s1, s0) and torch.equal(g1, g0)
    wide = torch.full((B, n + 7), float("nan"), dtype=dtype, device=DEV)
    wide[:, n + 1:] = 1e30
    wide[:, :n] = q
    yw, sw, gw = run(wide, gy)
    assert torch.equal(yw, y0) and torch.equal(sw, s0) and torch.equal(gw[:, :n], g0) and torch.all(gw[:, n:] == 0)
    qt = q.t().contiguous().t()                                # unit ROW stride
    assert qt.stride() == (1, B)
    yt, st, gt = run(qt, gy)
    assert torch.equal(yt, y0) and torch.equal(st, s0) and torch.equal(gt, g0)
    gy_wide = torch.full((B, k + 3), float("nan"), dtype=dtype, device=DEV)
    gy_wide[:, :k] = gy
    for view in (gy_wide[:, :k], gy.t().contiguous().t()):
        assert not view.is_contiguous()
        yv, sv, gv = run(q, view)
        assert torch.equal(yv, y0) and torch.equal(sv, s0) and torch.equal(gv, g0)


def _run(pack, call, q, gy):
    y, steps = ops.dc3_forward_raw(q, pack, call.lr, call.momentum, call.eps, call.max_steps)
    return y, steps, ops.dc3_backward_raw(q, steps, gy, pack, call.lr, call.momentum, call.max_steps)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_nonfinite_rows_keep_the_reference_semantics(dtype):
    case = ref.CASE["np16_n16_four_quadratics"]
    clean = ref.call_for(case.name, 257, 40, 7)                # alone, these rows stop after 7 of at most 40 steps
    pack = _pack(case.name, clean.arrays)
    pack.nan_flag.zero_()
    for value, row in ((float("nan"), 70), (float("inf"), 256)):
        q = clean.q.copy()
        q[row] = value
        with np.errstate(invalid="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            call = ref.evaluate(clean.arrays, q, clean.gy, clean.lr, clean.momentum, clean.eps, clean.max_steps)
        assert call.steps == call.steps32 == 40                # NaN < eps is false: the reference runs to the limit
        others = np.arange(257) != row
        _, steps, _ = _check(f"{case.name} row {row} = {value}", pack, call, dtype, rows=others)
        assert int(steps.item()) == 40
        assert int(pack.nan_flag.item()) == 1
        pack.nan_flag.zero_()
    _check(f"{case.name} clean again", pack, clean, dtype)
    assert int(pack.nan_flag.item()) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_equalities_only(dtype):
    """Without inequalities the reference never meets its stop rule (``stacked.numel()`` is 0) and runs to the limit."""
    case = ref.EQUALITIES_ONLY
    arrays = ref.make_pack(case)
    q, gy = ref.make_inputs(case, 65)
    for limit in (12, 40):
        call = ref.evaluate(arrays, q, gy, case.lr, ref.MOMENTUM, 1e-3, limit)
        assert call.steps == limit
        _check(case.name, _pack(case.name, arrays), call, dtype)


def test_equalities_only_module_counts_like_the_reference():
    raw = workloads._empty(5)
    rng = np.random.default_rng(12)
    raw["A2"] = rng.uniform(-1.0, 1.0, size=(2, 5))
    raw["b2"] = rng.uniform(-0.5, 0.5, size=(2, 1))
    raw["y0"] = np.linalg.lstsq(raw["A2"], raw["b2"], rcond=None)[0]
    args = dict(lr=1e-2, momentum=0.5, eps_converge=1e-3, max_steps_training=6, max_steps_testing=37)
    layer = ConstraintModule(workloads.build_constraints(raw), method="DC3", create_map=False, args_DC3=args).eval()
    q = torch.rand(65, 3, 1) - 0.5
    counts = {}
    for training in (False, True):
        layer.train(training)
        expect = layer(q)                                      # host tensors: the reference's formula
        counts[training] = layer.dc3_steps.tolist()
    layer = layer.to(DEV)
    for training in (False, True):
        layer.train(training)
        y = layer(q.to(DEV))
        assert layer.dc3_steps.tolist() == counts[training] and not layer._hip_unsupported
        assert dc3_cases.row_err(y.cpu()[:, :, 0], expect[:, :, 0]).max() <= 1e-5
