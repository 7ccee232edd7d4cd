"""Cases and calls for the DC3 tile kernels (rayen_amd/csrc/rayen_dc3_tile.hip): the reference, generators and bars of
tests/dc3_reference.py, four cases beyond the lane kernel's LDS image, and a kink rule widened for a kernel that sums in
another order than the host.

Kink rule.  The backward is discontinuous where a residual changes sign (``diag[r > 0]``).  ``dc3_reference.kink_rows``
leaves a row out where some residual is within ``4 |r32 - r64|`` of zero in the host's two runs; a kernel with another
summation order may disagree with fp64 on a residual the host's fp32 run happened to get nearly exact.  So here a row is
left out when, at any visited step, some residual has ``|r64| <= max(4 |r32 - r64|, F)``, F the largest ``|r32 - r64|`` over
ALL residuals of that call, or opposite signs in the two runs.  The number of rows left out stays capped at
``dc3_reference.kink_cap(B)``: a condition on the inputs (tests/test_dc3_tile_host.py shows it on the host), no tolerance.
"""
import functools

import numpy as np
import torch

import dc3_reference as ref

# name, n, m, nq, no, lr, amp; fp32 lane image in the comment (ref.lds_bytes)
TILE_CASES = [
    ref.LDS_CASE["lds_just_over"],                                           # 160 KiB, 256 B over
    ref.Case("tile_n33_forty_quadratics", 33, 40, 40, 2, 1e-3, 0.5),         # 661 KiB; two blocks of n with 31 padded rows,
                                                                             # non-symmetric Pe, 8 padded rows of A1e
    ref.Case("tile_n30_corridor_shape", 30, 1050, 72, 15, 5e-4, 0.5),        # 435 KiB; config 5's shape
    ref.Case("tile_n64_m2100_rows_only", 64, 2100, 0, 0, 4e-3, 0.5),         # 533 KiB; 66 row blocks, the last of 20 rows
]
TILE_CASE = {c.name: c for c in TILE_CASES}
CORRIDOR_SHAPE = (30, 1050, 72, 15)      # config 5 in DC3 form: n, effective rows, quadratics, eliminated variables

# (B, max_steps, t*) with forward and backward; forward only at B = 257 (t* None: eps = 0, a partial second launch)
BACKWARD_CALLS = [(33, 10, 7), (65, 10, 7), (33, 40, 33)]
FORWARD_CALLS = [(257, 10, 7), (257, 100, 33), (257, 33, None)]

# tile-mates, the NaN row
MATES_CASES = ["tile_n33_forty_quadratics", "np8_n5_ragged_everything"]
MATES_BATCHES = (1, 31, 32, 33, 65)
OUTLIER_BATCHES = (63, 64, 65)


def all_cases():
    return {**ref.CASE, **ref.LDS_CASE, **TILE_CASE}


def sweep_cases():
    """Every fp32 instance the lane kernel's sweep runs: ``ref.CASES`` and the served ``ref.LDS_CASES``."""
    return list(ref.CASES) + [c for c in ref.LDS_CASES if ref.served(c, torch.float32)]


def wide_kink_rows(res64, res32):
    """[B] bool: the widened rule of this file's docstring."""
    res64, res32 = np.asarray(res64, dtype=np.float64), np.asarray(res32, dtype=np.float64)
    if res64.size == 0:
        return np.zeros(res64.shape[1], dtype=bool)
    gap = np.abs(res32 - res64)
    near = np.abs(res64) <= np.maximum(ref.KINK_FACTOR * gap, np.max(gap))
    flipped = (res64 > 0) != (res32 > 0)
    return np.any(near | flipped, axis=(0, 2))


def largest_gap(call):
    f64, f32 = _forwards(call)
    return float(np.max(np.abs(f32.res - f64.res))) if f64.res.size and f32.steps == f64.steps else 0.0


def _forwards(call):
    return tuple(ref.forward_ref(call.arrays, call.q, call.lr, call.momentum, call.eps, call.max_steps, dt)
                 for dt in (torch.float64, torch.float32))


def widen(call):
    """``call`` (a ``ref.Call``) with its kink rows by the widened rule."""
    f64, f32 = _forwards(call)
    same = f32.steps == f64.steps
    kinks = wide_kink_rows(f64.res, f32.res) if same else np.ones(call.q.shape[0], dtype=bool)
    return call._replace(kinks=kinks | call.kinks)


@functools.lru_cache(maxsize=None)
def call_for(name, B, max_steps, t_star, seed=0):
    """``ref.call_for`` for every case of this file and of dc3_reference, with the widened kink rows."""
    if name in ref.CASE or name in ref.LDS_CASE:
        return widen(ref.call_for(name, B, max_steps, t_star, seed))
    case = TILE_CASE[name]
    arrays = ref.make_pack(case)
    q, gy = ref.make_inputs(case, B, seed)
    eps = 0.0
    if t_star is not None:
        eps = ref.eps_for(ref.forward_ref(arrays, q, case.lr, ref.MOMENTUM, 0.0, t_star).v, t_star)
    return widen(ref.evaluate(arrays, q, gy, case.lr, ref.MOMENTUM, eps, max_steps))


@functools.lru_cache(maxsize=None)
def forward_call_for(name, B, max_steps, t_star, seed=0):
    """A call whose forward alone is compared (every row): no host backward, no kinks."""
    case = all_cases()[name]
    arrays = ref.make_pack(case)
    q, gy = ref.make_inputs(case, B, seed)
    eps = 0.0
    if t_star is not None:
        eps = ref.eps_for(ref.forward_ref(arrays, q, case.lr, ref.MOMENTUM, 0.0, t_star).v, t_star)
    f64 = ref.forward_ref(arrays, q, case.lr, ref.MOMENTUM, eps, max_steps, torch.float64)
    f32 = ref.forward_ref(arrays, q, case.lr, ref.MOMENTUM, eps, max_steps, torch.float32)
    none = np.zeros((B, case.n))
    gap_y = float(np.max(ref.row_err(f32.y, f64.y)))
    return ref.Call(arrays, q, gy, case.lr, ref.MOMENTUM, eps, max_steps, f64.steps, f32.steps, f64.v, f64.y, none, f32.y, none,
                    gap_y, 0.0, np.zeros(B, dtype=bool))


@functools.lru_cache(maxsize=None)
def outlier_calls(B):
    """``ref.outlier_calls`` with the widened kink rows."""
    far, near = ref.outlier_calls(B)
    return widen(far), widen(near)


def sound(call, backward=True):
    """The conditions a call must meet on the host before a kernel is judged by it; returns what fails (empty: sound)."""
    said = []
    B = call.q.shape[0]
    if not (np.isfinite(call.y64).all() and np.isfinite(call.y32).all() and np.isfinite(call.v).all()):
        said.append("not finite")
    if call.steps != call.steps32:
        said.append(f"steps {call.steps} (fp64) != {call.steps32} (fp32)")
    if not ref.stop_margin(call.v, call.eps, call.steps, call.max_steps):
        said.append("the stop is decided within 0.5 % of eps")
    if backward:
        if not (np.isfinite(call.gq64).all() and np.isfinite(call.gq32).all()):
            said.append("gradient not finite")
        if int(call.kinks.sum()) > ref.kink_cap(B):
            said.append(f"{int(call.kinks.sum())} kink rows > cap {ref.kink_cap(B)}")
    return said
