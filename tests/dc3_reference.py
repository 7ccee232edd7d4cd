"""Reference, seeded cases and helpers for the sweep of the DC3 kernels (rayen_amd/csrc/rayen_dc3.hip).

The iteration is the one in the header comment of rayen_dc3.hip, written with plain torch ops on host tensors at the
dtype asked for (fp64 is the reference; the fp32 run of the same code gives the rounding gap the fp32 bar is made of):

    r = relu(A1e p - b1e),  g_i = 0.5 p'Pe_i p + qe_i'p + re_i,  u_i = Pe_i p + qe_i
    grad = 2 A1e' r + sum_i 2 u_i relu(g_i),   s <- lr grad + momentum s,   p <- p - s
    y[partial] = p,  y[other] = c0 + C p

with the reference's batch-global stop (after step t: stop when t reached the limit, else when the batch maximum of the
relu'd residuals is below eps; a set without inequalities never meets the second rule, as in ``dc3.reference_forward``
where ``stacked.numel()`` is 0).  The backward is torch autograd over the unrolled steps of that formula, NOT a
transcription of the kernel's hand-derived Jacobian: that derivation is what the sweep tests.

The sweep's cases and seeded generators live here too, so that tests/test_dc3_reference_host.py judges on the host the very
packs, inputs and stop positions tests/test_gpu_dc3_sweep.py runs on the GPU.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from dc3_cases import row_err

LDS_LIMIT = 160 * 1024 - 256        # bytes of image the kernels stage (rayen_dc3.hip: served())
KINK_FACTOR = 4.0


def pad_n(n):
    """NP of rayen_dc3_pack_create (0: beyond what the kernels stage)."""
    return 4 if n <= 4 else 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64 if n <= 64 else 0


def round4(x):
    return (x + 3) & ~3


def lds_bytes(case, elem):
    """Bytes of the LDS image of ``case`` at ``elem`` bytes per element (restates rayen_dc3.hip: dims_of)."""
    NP = pad_n(case.n)
    total = case.m * NP + round4(case.m) + case.nq * (NP * NP + NP + 4) + case.no * NP + round4(case.no) + 4
    return total * elem


def served(case, dtype):
    elem = 4 if dtype == torch.float32 else 8
    return 0 < pad_n(case.n) <= (64 if elem == 4 else 32) and lds_bytes(case, elem) <= LDS_LIMIT


def kink_cap(B):
    """The cap of tests/test_gpu_backward.py on rows left out of a backward comparison."""
    return max(2, int(0.02 * B))


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------

# lr and the input amplitude are per case: the fp64 host iteration stays finite on every row over 100 steps, the batch
# violation falls by more than 1 % per step at every stop target the case is used with, and the kink share stays within
# the cap (tests/test_dc3_reference_host.py shows all three on the host).
Case = namedtuple("Case", "name n m nq no lr amp")

# name: np<NP>_n<n>_<what it is there for>.  Every NP with padding lanes (n < NP) and full (n == NP).
CASES = [
    Case("np4_n1_one_inequality", 1, 1, 0, 0, 1e-2, 1.5),                # nq = 0 with m > 0; three padding lanes
    Case("np4_n4_quadratics_only", 4, 0, 3, 1, 5e-3, 1.0),               # m = 0 with nq > 0: off_q == 0; non-symmetric Pe
    Case("np8_n5_ragged_everything", 5, 5, 1, 3, 1e-2, 1.5),             # m % 4 = 1 in front of off_q, round4(no) = 4 > no
    Case("np8_n8_three_quadratics", 8, 6, 3, 0, 1e-2, 1.0),              # m % 4 = 2 in front of off_q, symmetric Pe
    Case("np16_n9_inequalities_only", 9, 48, 0, 5, 1e-2, 1.0),           # nq = 0, no = 5 rows of C (round4 = 8)
    Case("np16_n16_four_quadratics", 16, 5, 4, 1, 5e-3, 1.0),            # m % 4 = 1, four non-symmetric Pe
    Case("np32_n17_one_quadratic", 17, 6, 1, 5, 1e-2, 1.0),              # 15 padding lanes, m % 4 = 2
    Case("np32_n32_full", 32, 48, 3, 3, 4e-3, 0.5),                      # the forward that spills most (fp32), no = 3
    Case("np64_n33_nearly_unconstrained", 33, 1, 1, 0, 1e-2, 0.5),       # 31 padding lanes, m = nq = 1
    Case("np64_n64_five_equalities", 64, 5, 3, 5, 2e-3, 0.5),           # NP = 64 with non-symmetric Pe and C
    Case("np64_n64_c3_shape", 64, 128, 4, 0, 1e-3, 0.25),                # the c3 shape: the backward that spills most
]
CASE = {c.name: c for c in CASES}

# one case per NP for the stop-position matrix
POSITION_CASES = ["np4_n4_quadratics_only", "np8_n5_ragged_everything", "np16_n16_four_quadratics", "np32_n32_full",
                  "np64_n64_five_equalities"]

# images that reach the dynamic-LDS opt-in and the limit of served() (bytes: see test_dc3_reference_host.py)
LDS_CASES = [
    Case("lds_above_48k", 32, 400, 1, 0, 3e-3, 0.5),                     # fp32 image 55.7 KiB (fp64 111.4 KiB: served too)
    Case("lds_at_the_limit", 64, 565, 1, 0, 2e-3, 0.25),                 # fp32 image == 160 KiB - 256 B exactly
    Case("lds_just_over", 64, 566, 1, 0, 2e-3, 0.25),                    # one more row: 256 B over
    Case("lds_fp32_only", 32, 700, 0, 1, 2e-3, 0.5),                     # fp32 90.4 KiB fits, fp64 180.8 KiB does not
]
LDS_CASE = {c.name: c for c in LDS_CASES}

EQUALITIES_ONLY = Case("np8_n6_equalities_only", 6, 0, 0, 3, 1e-2, 1.0)

MOMENTUM = 0.5
TRAIN_CALL = (10, 7)                # (max_steps, t*): tstar < max_steps, the backward workspace is sized by the limit
EVAL_CALL = (64, 45)
SWEEP_BATCHES = (1, 65, 257)
POSITION_BATCH = 257
# (max_steps, t*); t* None: eps = 0, never stops and ends in a partial last chunk (or exactly at a chunk's end)
POSITIONS = [(1, 1), (32, 32), (33, 33), (33, 32), (100, 1), (100, 2), (100, 31), (100, 32), (100, 33), (100, 64),
             (100, 65), (100, 96), (100, 97), (32, None), (33, None), (100, None)]


def _seed(case, *extra):
    return [case.n, case.m, case.nq, case.no, *extra]


def _f32(x):
    """fp64 array of fp32-representable values: both images of a pack and both host runs start from the same numbers."""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64))


def make_pack(case, center=None):
    """The dict ``ops.Dc3Pack`` takes (keys of ``rayen_amd/dc3.py::pack_arrays``), built directly in R^n.

    ``A1e`` rows of norm 0.8 .. 1.2, ``b1e`` in (0.3, 0.5); ``Pe_i = M M' + 0.1 I`` plus, when the set has equalities, a
    non-symmetric part (the reference's effective P is not symmetric there); ``re_i`` in (-0.6, -0.4); dense ``C`` and
    ``c0``; ``partial`` / ``other`` an interleaved permutation of range(k).  The origin is strictly inside.  With
    ``center`` the same set is translated to ``center`` (the origin, where the kernels' inactive lanes sit, is then
    outside when ``center`` is far enough)."""
    n, m, nq, no = case.n, case.m, case.nq, case.no
    rng = np.random.default_rng(_seed(case, 1))
    A = rng.standard_normal((m, n))
    A *= (rng.uniform(0.8, 1.2, size=(m, 1)) / np.maximum(np.linalg.norm(A, axis=1, keepdims=True), 1e-300))
    b = rng.uniform(0.3, 0.5, size=m)
    Pe = np.zeros((nq, n, n))
    for i in range(nq):
        M = rng.standard_normal((n, n)) / np.sqrt(n)
        Pe[i] = M @ M.T + 0.1 * np.eye(n)
        if no > 0:
            Pe[i] += 0.3 * rng.standard_normal((n, n)) / np.sqrt(n)
    qe = 0.2 * rng.standard_normal((nq, n)) / np.sqrt(n)
    re = -rng.uniform(0.4, 0.6, size=nq)
    C = rng.standard_normal((no, n)) / np.sqrt(n)
    c0 = rng.standard_normal(no)
    perm = rng.permutation(n + no)
    if center is not None:
        c = np.asarray(center, dtype=np.float64).reshape(n)
        b = b + A @ c
        for i in range(nq):                                # g(p - c)
            re[i] = re[i] + 0.5 * c @ Pe[i] @ c - qe[i] @ c
            qe[i] = qe[i] - 0.5 * (Pe[i] + Pe[i].T) @ c
    return dict(A1e=_f32(A).reshape(m, n), b1e=_f32(b), Pe=_f32(Pe).reshape(nq, n, n), qe=_f32(qe).reshape(nq, n),
                re=_f32(re), C=_f32(C).reshape(no, n), c0=_f32(c0),
                partial=np.ascontiguousarray(perm[:n], dtype=np.int32),
                other=np.ascontiguousarray(perm[n:], dtype=np.int32), n=n, k=n + no)


def make_inputs(case, B, seed=0, amplitude=None):
    """(q [B, n], gy [B, k]) as fp64 arrays of fp32-representable values: q uniform in +-amplitude (the case's by
    default), gy standard normal."""
    rng = np.random.default_rng(_seed(case, 2, B, seed))
    amp = case.amp if amplitude is None else amplitude
    q = rng.uniform(-amp, amp, size=(B, case.n))
    gy = rng.standard_normal(size=(B, case.n + case.no))
    return _f32(q), _f32(gy)


# ------------------------------------------------------------------------------------------------------------------
# the iteration
# ------------------------------------------------------------------------------------------------------------------

def _constants(arrays, dtype):
    t = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64)).to(dtype)        # noqa: E731
    n, k = int(arrays["n"]), int(arrays["k"])
    perm = np.concatenate([np.asarray(arrays["partial"]).reshape(-1), np.asarray(arrays["other"]).reshape(-1)])
    inverse = np.empty(k, dtype=np.int64)
    inverse[perm.astype(np.int64)] = np.arange(k)
    return dict(A=t(arrays["A1e"]).reshape(-1, n), b=t(arrays["b1e"]).reshape(-1), P=t(arrays["Pe"]).reshape(-1, n, n),
                q=t(arrays["qe"]).reshape(-1, n), r=t(arrays["re"]).reshape(-1), C=t(arrays["C"]).reshape(-1, n),
                c0=t(arrays["c0"]).reshape(-1), inverse=torch.as_tensor(inverse), n=n, k=k)


def _residuals(c, p):
    """(lin [B, m], g [B, nq], u [B, nq, n]) at p [B, n]."""
    lin = p @ c["A"].t() - c["b"]
    Pp = torch.einsum("cjl,bl->bcj", c["P"], p)
    g = 0.5 * torch.einsum("bcj,bj->bc", Pp, p) + p @ c["q"].t() + c["r"]
    return lin, g, Pp + c["q"]


def _step(c, p, s, lr, momentum, parts=None):
    lin, g, u = _residuals(c, p) if parts is None else parts
    grad = 2.0 * (torch.relu(lin) @ c["A"]) + 2.0 * torch.einsum("bc,bcj->bj", torch.relu(g), u)
    s = lr * grad + momentum * s
    return p - s, s


def _assemble(c, p):
    return torch.cat([p, c["c0"] + p @ c["C"].t()], dim=1)[:, c["inverse"]]


def _batch_violation(res):
    """Batch maximum of the relu'd residuals (NaN kept, as torch.max keeps it); 0 for a set without inequalities."""
    return float(torch.max(torch.relu(res))) if res.numel() else 0.0


Forward = namedtuple("Forward", "y steps v res")


def forward_ref(arrays, q, lr, momentum, eps, max_steps, dtype=torch.float64):
    """``Forward(y [B, k], steps, v [steps + 1], res [steps + 1, B, m + nq])`` as fp64 numpy arrays: ``v[t]`` is the batch
    violation after step t (``v[0]``: of the input, which the stop rule never reads), ``res[t]`` every residual
    (``A1e p - b1e``, then ``g_i``) at ``p_t``."""
    c = _constants(arrays, dtype)
    with torch.no_grad():
        p = torch.as_tensor(np.asarray(q, dtype=np.float64))[:, :c["n"]].to(dtype)
        s = torch.zeros_like(p)
        all_res, v, steps = [], [], 0
        never = c["A"].shape[0] + c["P"].shape[0] == 0
        while True:
            parts = _residuals(c, p)
            res = torch.cat(parts[:2], dim=1)
            all_res.append(res)
            v.append(_batch_violation(res))
            if steps >= max_steps or (steps >= 1 and not never and v[-1] < eps):
                break
            p, s = _step(c, p, s, lr, momentum, parts)
            steps += 1
        y = _assemble(c, p)
    return Forward(y.double().numpy(), steps, np.asarray(v, dtype=np.float64), torch.stack(all_res).double().numpy())


def backward_ref(arrays, q, gy, lr, momentum, steps, dtype=torch.float64):
    """``d <gy, y> / dq`` [B, n] by torch autograd over the ``steps`` unrolled steps of the forward formula."""
    c = _constants(arrays, dtype)
    p0 = torch.as_tensor(np.asarray(q, dtype=np.float64))[:, :c["n"]].to(dtype).clone().requires_grad_(True)
    p, s = p0, torch.zeros_like(p0)
    for _ in range(int(steps)):
        p, s = _step(c, p, s, lr, momentum)
    y = _assemble(c, p)
    (grad,) = torch.autograd.grad((y * torch.as_tensor(np.asarray(gy, dtype=np.float64)).to(dtype)).sum(), p0)
    return grad.double().numpy()


def eps_for(v, t_star):
    """An eps that makes the iteration stop at ``t_star`` with at least 0.5 % to spare on both sides: the geometric mean of
    ``v[t_star]`` and the smallest earlier violation (for ``t_star == 1`` there is none: the violation of the input)."""
    before = float(np.min(v[1:t_star])) if t_star > 1 else float(v[0])
    here = float(v[t_star])
    assert np.isfinite(here) and np.isfinite(before) and 0.0 < here < 0.99 * before, (t_star, here, before)
    return float(np.sqrt(here * before))


def kink_rows(res64, res32):
    """[B] bool: rows where at any visited step some residual is within ``4 |r32 - r64|`` of zero, or has opposite signs in
    the two host runs.  The backward is discontinuous there (``diag[r > 0]``); the forward is not."""
    res64, res32 = np.asarray(res64, dtype=np.float64), np.asarray(res32, dtype=np.float64)
    near = np.abs(res64) <= KINK_FACTOR * np.abs(res32 - res64)
    flipped = (res64 > 0) != (res32 > 0)
    return np.any(near | flipped, axis=(0, 2))


# ------------------------------------------------------------------------------------------------------------------
# one call of the sweep: inputs, eps, both host runs (computed once, shared by the host and the GPU tests)
# ------------------------------------------------------------------------------------------------------------------

Call = namedtuple("Call", "arrays q gy lr momentum eps max_steps steps steps32 v y64 gq64 y32 gq32 gap_y gap_g kinks")


def evaluate(arrays, q, gy, lr, momentum, eps, max_steps):
    """Both host runs of one call."""
    f64 = forward_ref(arrays, q, lr, momentum, eps, max_steps, torch.float64)
    f32 = forward_ref(arrays, q, lr, momentum, eps, max_steps, torch.float32)
    g64 = backward_ref(arrays, q, gy, lr, momentum, f64.steps, torch.float64)
    g32 = backward_ref(arrays, q, gy, lr, momentum, f64.steps, torch.float32)
    same = f32.steps == f64.steps
    kinks = kink_rows(f64.res, f32.res) if same else np.ones(q.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        gap_y = float(np.max(row_err(f32.y, f64.y)))
        gap_g = float(np.max(row_err(g32, g64)[~kinks])) if not kinks.all() else 0.0
    return Call(arrays, q, gy, lr, momentum, eps, max_steps, f64.steps, f32.steps, f64.v, f64.y, g64, f32.y, g32, gap_y, gap_g, kinks)


def gaps(call, rows_y=None, rows_g=None):
    """The host fp32-versus-fp64 gap of ``call`` (``y``, ``grad_q``): the maximum of ``row_err`` over the rows given (all rows,
    and all rows outside the kinks, by default)."""
    rows_y = np.ones(call.q.shape[0], dtype=bool) if rows_y is None else rows_y
    rows_g = ~call.kinks if rows_g is None else rows_g
    gap_y = float(np.max(row_err(call.y32[rows_y], call.y64[rows_y]))) if rows_y.any() else 0.0
    gap_g = float(np.max(row_err(call.gq32[rows_g], call.gq64[rows_g]))) if rows_g.any() else 0.0
    return gap_y, gap_g


def _all_cases():
    return {**CASE, **LDS_CASE, EQUALITIES_ONLY.name: EQUALITIES_ONLY}


@functools.lru_cache(maxsize=None)
def call_for(name, B, max_steps, t_star, seed=0):
    """The sweep's call of case ``name``: eps placed so that the fp64 host run stops at ``t_star`` (None: eps = 0)."""
    case = _all_cases()[name]
    arrays = make_pack(case)
    q, gy = make_inputs(case, B, seed)
    eps = 0.0
    if t_star is not None:
        eps = eps_for(forward_ref(arrays, q, case.lr, MOMENTUM, 0.0, t_star).v, t_star)
    return evaluate(arrays, q, gy, case.lr, MOMENTUM, eps, max_steps)


def stop_margin(v, eps, steps, max_steps):
    """True when the stop of a run with violations ``v`` is decided at least 0.5 % away from ``eps`` on both sides."""
    if np.any(v[1:steps] < 1.005 * eps):
        return False
    return steps == max_steps or v[steps] < 0.995 * eps


# the deciding row of test_deciding_row_in_the_last_partial_wave
OUTLIER_CASE = "np8_n5_ragged_everything"
OUTLIER_BATCHES = (63, 64, 65, 255, 256, 257, 513)
OUTLIER_CALL = (64, 40)


@functools.lru_cache(maxsize=None)
def outlier_calls(B):
    """(with, without): the set of OUTLIER_CASE translated away from the origin (the kernels' inactive lanes sit at the
    origin, which is then OUTSIDE the set by more than any eps used); every row drawn close to the centre, inside the set;
    in ``with``, row B - 1 far outside, so that it alone holds the violation above eps until step 40."""
    case = CASE[OUTLIER_CASE]
    center = np.full(case.n, 3.0) * np.where(np.arange(case.n) % 2 == 0, 1.0, -1.0)
    arrays = make_pack(case, center=center)
    small, gy = make_inputs(case, B, seed=7, amplitude=0.05)
    inside = _f32(small + center)
    far = inside.copy()
    far[B - 1] = _f32(center + make_inputs(case, 1, seed=8, amplitude=1.0)[0][0] * 2.0)
    max_steps, t_star = OUTLIER_CALL
    eps = eps_for(forward_ref(arrays, far, case.lr, MOMENTUM, 0.0, t_star).v, t_star)
    return (evaluate(arrays, far, gy, case.lr, MOMENTUM, eps, max_steps),
            evaluate(arrays, inside, gy, case.lr, MOMENTUM, eps, max_steps))
