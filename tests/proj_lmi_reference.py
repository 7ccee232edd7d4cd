"""fp64 reference, seeded cases and helpers for the Euclidean projection onto sets WITH AN LMI (the PSD block of
rayen_amd/csrc/rayen_proj.hip and of the mirror in rayen_amd/projection.py, both behind ``lmi=True``).

Forward reference: ``proj_reference.project_rows`` as it is (``conic.solve`` per row at 1e-11 on the unequilibrated program,
the PSD block in full ``r x r`` storage: another implementation than the fixed-``rho`` svec iteration under test).

Backward reference: the KKT Jacobian from the ORIGINAL constraint functions, extended to ``F(y) = F_k + sum_a y_a F_a >= 0``
at ``y = NA_E z + yp``.  With ``U`` the null basis of ``F(y*)`` (eigenvalues below ACTIVE_TOL, ``p`` of them) and ``F^+`` the
pseudo-inverse on the rest:

    tangent rows        Ja_ij = [u_i' F_a u_j]_a NA_E                         for i <= j <= p
    multiplier          Lambda = U M U',  z* - q = NA_E' [<F_a, Lambda>]_a    (M symmetric, fitted by least squares together
                                                                               with the multipliers of the other active rows)
    curvature           H += 2 NA_E' [tr(Lambda F_a F^+ F_b)]_ab NA_E
    J = H^-1 - H^-1 Ja' (Ja H^-1 Ja')^+ Ja H^-1

The margin of a row takes in ``lambda_min(M)`` and the smallest eigenvalue of ``F(y*)`` outside the null space; below
KINK_MARGIN the row is a kink row.  tests/test_proj_lmi_reference_host.py holds this Jacobian against central finite
differences of ``project_rows``.

The bars follow proj_reference: KINK_FACTOR times the gap of the host mirror at that precision against the fp64 reference on
the same inputs, never the kernel's own gap; in fp64 no looser than FP64_CAP.
"""
import functools
from collections import namedtuple

import numpy as np

import proj_reference as pr
from proj_reference import (ACTIVE_TOL, EPS, FP64_CAP, KINK_FACTOR, KINK_MARGIN, LDS_LIMIT, MAX_N, MAX_ROWS, MAX_SOC,  # noqa: F401
                            WAVES, kink_cap, project_rows, round4, row_gap)
from rayen_amd import workloads

BATCHES = (1, 65, 257)
MAX_PSD = 32                         # rayen_proj.hip: kMaxPsd
MAX_ITERS = 4096
DECISION_MARGIN = 1e-4               # no seeded row has |lambda_min(F(q))| below this times (1 + ||F(q)||)


def psd_scratch(r):
    """Elements of per-wave LDS scratch the PSD block adds (rayen_proj.hip: dims_of)."""
    return 96 + 3 * round4(r * (r | 1)) if r else 0


def lds_bytes(n, m, r, elem):
    mpad = m | 1
    image = round4(n * mpad) + round4(n * n) + round4(m) + round4(n)
    return (image + WAVES * (128 + round4(m) + psd_scratch(r))) * elem


def served(n, m, n_soc, r, elem):
    """Restates the kernel's rule (rayen_proj.hip: shape_served) for a program with an ``r x r`` PSD block."""
    return (1 <= n <= MAX_N and 1 <= m <= MAX_ROWS and n_soc <= MAX_SOC and 0 <= r <= MAX_PSD
            and lds_bytes(n, m, r, elem) <= LDS_LIMIT)


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------

# rho: None lets build_program choose it (every small case does); the three large blocks carry the value it chose on the
# host, because its probing there (7 candidates x up to 2000 iterations of eigh) takes 1 to 2 minutes that the tests need
# not repeat
Case = namedtuple("Case", "name raw amp batch rho seed", defaults=(257, None, 0))


def _raw_half_line():
    raw = workloads._empty(1)
    raw["F"] = [np.array([[1.0]]), np.array([[1.0]])]                        # y + 1 >= 0
    return raw


def _raw_psd_cone():
    """``F(y) = [[y1, y2/sqrt2], [y2/sqrt2, y3]]``: y IS svec(F), so the projection is svec(Pi_psd(smat(q)))."""
    s = 1.0 / np.sqrt(2.0)
    raw = workloads._empty(3)
    raw["F"] = [np.array([[1.0, 0.0], [0.0, 0.0]]), np.array([[0.0, s], [s, 0.0]]), np.array([[0.0, 0.0], [0.0, 1.0]]),
                np.zeros((2, 2))]
    raw["y0"] = np.array([[1.0], [0.0], [1.0]])
    return raw


def _raw_identity_offset():
    """``F_k = I`` and generators of size 0.1: every eigenvalue of ``F`` near 1 (a cluster) until ``|y|`` is large."""
    rng = np.random.default_rng(66)
    raw = workloads._empty(5)
    for _ in range(5):
        T = rng.uniform(-1.0, 1.0, (6, 6))
        raw["F"].append(0.1 * (T + T.T) / 2)
    raw["F"].append(np.eye(6))
    return raw


def _raw_eq_lin_lmi():
    rng = np.random.default_rng(835)
    raw = workloads.random_lmi(8, 5, seed=835)
    raw["A1"], raw["b1"] = rng.uniform(-1, 1, (5, 8)), rng.uniform(0.3, 1.0, (5, 1))
    raw["A2"], raw["b2"] = rng.uniform(-1, 1, (3, 8)), np.zeros((3, 1))
    return raw


def _raw_quad_soc_lmi():
    raw = workloads.random_lin_quad_soc(6, 3, 1, 1, seed=7)
    raw["F"] = workloads.random_lmi(6, 7, seed=77)["F"]
    return raw


def _rlmi(k, r, seed=0):
    return lambda: workloads.random_lmi(k, r, seed=seed)


CASES = [
    Case("r1_k1", _raw_half_line, 1.5),                              # an LMI that is a half-line; no rotation at all
    Case("r2_psd_cone_isometric", _raw_psd_cone, 1.5),               # known answer in closed form
    Case("r3_k4", _rlmi(4, 3, seed=1), 1.5),                         # odd r: the padded round-robin
    Case("r6_identity_offset", _raw_identity_offset, 12.0),          # eigenvalues cluster at 1; rows leave the set
    Case("r8_k6", _rlmi(6, 8, seed=0), 3.0),                         # nullity-2 rows in the batch
    Case("k8_eq3_lin5_lmi5", _raw_eq_lin_lmi, 1.0),                  # NA_E != I, orthant rows and the block
    Case("quad_soc_lmi7", _raw_quad_soc_lmi, 0.5),                   # the block after SOCs, psd_row0 = 18
    Case("r20_k10", _rlmi(10, 20, seed=0), 1.5, 65, 10.0),               # config 4's shape: 210 rows, 4 per lane
    Case("r32_k4", _rlmi(4, 32, seed=0), 1.5, 65, 3.0),                 # the largest served: 528 rows, 9 per lane
]
REFUSED = Case("r33_refused", _rlmi(2, 33, seed=0), 1.5, 9, 3.0)        # served() false: the mirror and its warning
CASE = {c.name: c for c in CASES + [REFUSED]}

# (n, cone rows m, cones, r) of each case's program (tests/test_proj_lmi_reference_host.py holds them against the programs)
SHAPE = {"r1_k1": (1, 1, 0, 1), "r2_psd_cone_isometric": (3, 3, 0, 2), "r3_k4": (4, 6, 0, 3),
         "r6_identity_offset": (5, 21, 0, 6), "r8_k6": (6, 36, 0, 8), "k8_eq3_lin5_lmi5": (5, 20, 0, 5),
         "quad_soc_lmi7": (6, 46, 2, 7), "r20_k10": (10, 210, 0, 20), "r32_k4": (4, 528, 0, 32),
         "r33_refused": (2, 561, 0, 33)}


def batches_of(name):
    return tuple(B for B in BATCHES if B <= CASE[name].batch)


@functools.lru_cache(maxsize=None)
def make_cs(name):
    return workloads.build_constraints(CASE[name].raw())


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64))


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """``(q [B, n], gy [B, k])``, fp64 arrays of fp32-representable values; a smaller batch is the leading rows.
    ``q = z0 + amp u N(0, I)`` with ``u`` uniform in (0, 1.5) per row: interior, shallow and deep rows in every batch."""
    cs, case = make_cs(name), CASE[name]
    rng = np.random.default_rng([cs.n, cs.k, len(name), 11, case.seed])
    q = cs.z0.reshape(1, -1) + case.amp * rng.uniform(0.0, 1.5, (case.batch, 1)) * rng.standard_normal((case.batch, cs.n))
    gy = rng.standard_normal((case.batch, cs.k))
    return _f32(q), _f32(gy)


# ------------------------------------------------------------------------------------------------------------------
# backward reference
# ------------------------------------------------------------------------------------------------------------------

def lmi_matrix(cs, z):
    """``(F(y) [r, r], [F_a] [k, r, r])`` at ``y = NA_E z + yp``."""
    Fa = np.stack([np.asarray(F, dtype=np.float64) for F in cs.lmic.all_F[:-1]], axis=0)
    y = (cs.NA_E @ z.reshape(-1, 1) + cs.yp).ravel()
    return np.asarray(cs.lmic.all_F[-1], dtype=np.float64) + np.einsum("a,aij->ij", y, Fa), Fa


def decision_margin(cs, q):
    """``|lambda_min(F(q))| / (1 + ||F(q)||)``: how far the interior-or-not decision of the block is from a coin toss."""
    F, _ = lmi_matrix(cs, q)
    return abs(float(np.linalg.eigvalsh(F)[0])) / (1.0 + float(np.linalg.norm(F)))


def jacobian_row(cs, q, z):
    """``(J [n, n], margin, nullity)`` of the projection at ``q`` (solution ``z``); see the module docstring."""
    n, N = cs.n, cs.NA_E
    g = pr.constraint_values(cs, z)
    active = np.flatnonzero(g >= -ACTIVE_TOL)
    slack = -g[g < -ACTIVE_TOL]
    margin = float(slack.min()) if slack.size else np.inf
    F, Fa = lmi_matrix(cs, z)
    lam, W = np.linalg.eigh(F)
    null = lam < ACTIVE_TOL
    p = int(np.count_nonzero(null))
    if p < lam.size:
        margin = min(margin, float(lam[~null].min()))
    if (active.size == 0 and p == 0) or float(np.max(np.abs(q - z))) <= ACTIVE_TOL:
        if active.size or p:             # on the boundary with a zero step: multipliers 0
            margin = 0.0
        return np.eye(n), margin, p
    parts = [pr.constraint_derivatives(cs, z, int(i)) for i in active]
    rows = [part[0] for part in parts]
    cols = [r.T for r in rows]           # columns of the stationarity system  q - z = sum_i lambda_i grad g_i - NA_E'[<F_a, Lambda>]
    U = W[:, null]
    pairs = [(i, j) for i in range(p) for j in range(i, p)]
    if p:
        T = np.stack([np.einsum("r,ars,s->a", U[:, i], Fa, U[:, j]) @ N for i, j in pairs], axis=0)      # [pairs, n]
        rows.append(T)
        cols.append(-(T * np.array([1.0 if i == j else 2.0 for i, j in pairs])[:, None]).T)
    Ja = np.concatenate(rows, axis=0)
    mult = np.linalg.lstsq(np.concatenate(cols, axis=1), q - z, rcond=None)[0]
    H, at = np.eye(n), 0
    for r, hess, apex in parts:
        l = mult[at:at + r.shape[0]]
        at += r.shape[0]
        if apex:
            margin = min(margin, float(l[-1] - np.linalg.norm(l[:-1])))
        else:
            margin = min(margin, float(l[0]))
            H = H + l[0] * hess
    if p:
        M = np.zeros((p, p))
        for (i, j), x in zip(pairs, mult[at:]):
            M[i, j] = M[j, i] = x
        margin = min(margin, float(np.linalg.eigvalsh(M)[0]))
        Lam = U @ M @ U.T
        Fp = (W[:, ~null] / lam[~null]) @ W[:, ~null].T
        C = np.einsum("ij,ajk,kl,bli->ab", Lam, Fa, Fp, Fa)
        H = H + 2.0 * N.T @ (0.5 * (C + C.T)) @ N
    Hi = np.linalg.inv(H)
    S = Ja @ Hi @ Ja.T
    J = Hi - Hi @ Ja.T @ np.linalg.pinv(S, rcond=1e-10) @ Ja @ Hi
    return J, margin, p


Reference = namedtuple("Reference", "q gy z grad_q margin kink interior nullity")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The seeded batch of ``name`` solved once: ``z``, ``grad_q = J NA_E' gy``, the kink margins, the nullities."""
    cs = make_cs(name)
    q, gy = make_inputs(name)
    z = project_rows(cs, q)
    gz = gy @ cs.NA_E
    grad, margin, nullity = np.empty_like(q), np.empty(q.shape[0]), np.empty(q.shape[0], dtype=np.int64)
    for b in range(q.shape[0]):
        J, margin[b], nullity[b] = jacobian_row(cs, q[b], z[b])
        grad[b] = J @ gz[b]
    interior = np.array([float(np.max(pr.constraint_values(cs, q[b]), initial=-np.inf)) <= 0.0
                         and float(np.linalg.eigvalsh(lmi_matrix(cs, q[b])[0])[0]) >= 0.0 for b in range(q.shape[0])])
    for r in (z, grad, margin, interior, nullity):
        r.setflags(write=False)
    return Reference(q, gy, z, grad, margin, margin < KINK_MARGIN, interior, nullity)


# ------------------------------------------------------------------------------------------------------------------
# the host mirror on the seeded batches, and the bars made of it
# ------------------------------------------------------------------------------------------------------------------

# Measured on the host, the seeded batch of each case, row_gap against the reference (forward / backward on non-kink rows),
# iterations (max / mean) of the mirror at its chosen rho, kink rows, the largest nullity of F(y*) in the batch and the
# smallest decision margin |lambda_min(F(q))| / (1 + ||F(q)||):
#   case                    rho   fp64 eps 1e-9: fwd   bwd      iters            fp32 eps 1e-6: fwd   bwd      iters        inside    kink  nullity  margin
#   r1_k1                    10    7.0e-10  8.4e-13    17 /   1.9      4.2e-07  6.8e-07     9 /   1.2    218 / 257   0     1      2.4e-02
#   r2_psd_cone_isometric     3    3.2e-10  4.8e-10    17 /   5.1      7.9e-07  5.5e-07     6 /   2.2    150 / 257   0     2      5.8e-03
#   r3_k4                     3    3.0e-09  9.3e-09   111 /  21.0      3.5e-06  8.0e-06    66 /  12.9    116 / 257   0     2      8.2e-04
#   r6_identity_offset       10    1.2e-08  4.8e-08  1538 / 134.5      1.9e-05  9.6e-05   801 /  79.4     53 / 257   0     2      1.6e-03
#   r8_k6                     3    1.6e-08  1.3e-07  3546 / 151.9      2.0e-05  1.4e-04  1745 /  85.7     31 / 257   0     3      8.0e-04
#   k8_eq3_lin5_lmi5          3    6.2e-09  1.9e-08   232 /  40.1      7.6e-06  1.7e-05   125 /  23.8     85 / 257   0     2      4.5e-04
#   quad_soc_lmi7             3    9.4e-09  4.5e-08   107 /  54.3      8.4e-06  4.0e-05    65 /  31.4     72 / 257   0     1      1.3e-04
#   r20_k10                  10    3.2e-08  5.6e-08   312 / 179.0      3.3e-05  7.3e-05   180 / 102.8      5 /  65   0     3      5.6e-03
#   r32_k4                    3    9.6e-08  4.1e-07  1118 / 299.2      9.1e-05  3.9e-04   516 / 150.0      9 /  65   0     2      7.0e-04
# (rho as build_program chose it; MAX_ITERS is 4096 because the slowest rows of r8_k6 need 3546 in fp64.  The fp32 figures
# depend a little on the host's LAPACK; the bars are made of the run on the machine that tests.  With the block rebuilt as
# V max(lambda, 0) V' instead of v - V min(lambda, 0) V' the fp32 mirror of r32_k4 measured 4.6e-05 / 1.7e-04 and
# 614 / 198.3 on one host, and 3759 iterations on its slowest row on another: see projection._psd_project.)


@functools.lru_cache(maxsize=None)
def module_for(name):
    from rayen_amd import projection
    return projection.ProjectionModule(make_cs(name), create_map=False, lmi=True, rho=CASE[name].rho)


def shape_of(name):
    prog = module_for(name).program
    return prog.n, prog.m, len(prog.soc_rows), prog.psd_dim


def case_served(name, dtype_name):
    return served(*SHAPE[name], 4 if dtype_name == "float32" else 8)


Run = namedtuple("Run", "z grad_q iters")


def run_mirror(module, name, dtype_name, max_iters=MAX_ITERS, eps=None):
    """The mirror of ``module`` on the seeded batch of ``name`` at ``dtype_name``."""
    import torch
    from rayen_amd import projection
    dtype = getattr(torch, dtype_name)
    cs = make_cs(name)
    q, gy = make_inputs(name)
    c = projection.Constants(module.program, dtype, torch.device("cpu"))
    eps = EPS[dtype_name] if eps is None else eps
    z, iters, vstar = projection.mirror_forward(c, torch.from_numpy(q).to(dtype), max_iters, eps)
    g = torch.from_numpy(gy @ cs.NA_E).to(dtype)
    grad = projection.mirror_backward(c, g, vstar, iters, max_iters, eps)
    return Run(z.double().numpy(), grad.double().numpy(), iters.numpy())


@functools.lru_cache(maxsize=None)
def mirror_run(name, dtype_name):
    return run_mirror(module_for(name), name, dtype_name)


@functools.lru_cache(maxsize=None)
def bars(name, dtype_name):
    """``(forward bar, backward bar, violation bar)``: proj_reference.bars on these cases."""
    ref, run = reference(name), mirror_run(name, dtype_name)
    ok = ~ref.kink
    fwd = KINK_FACTOR * float(row_gap(run.z, ref.z).max())
    bwd = KINK_FACTOR * float(row_gap(run.grad_q, ref.grad_q)[ok].max())
    cs = make_cs(name)
    viol = KINK_FACTOR * max(float(np.max(cs.getViolationRows(run.z @ cs.NA_E.T + cs.yp.T))), 0.0)
    tiny = 64 * np.finfo(np.float32 if dtype_name == "float32" else np.float64).eps
    if dtype_name == "float64":
        fwd, bwd = min(fwd, FP64_CAP), min(bwd, FP64_CAP)
    return max(fwd, tiny), max(bwd, tiny), max(viol, tiny)


def compare(name, dtype_name, z, grad_q, iters, rows=None):
    """``proj_reference.compare`` on these cases: a list of failures (empty: passed).  ``rows``: the leading rows given."""
    ref, cs = reference(name), make_cs(name)
    B = len(z) if rows is None else rows
    fwd_bar, bwd_bar, viol_bar = bars(name, dtype_name)
    z, grad_q, iters = np.asarray(z, dtype=np.float64), np.asarray(grad_q, dtype=np.float64), np.asarray(iters)
    fails = []
    gap = row_gap(z, ref.z[:B])
    if not np.all(gap <= fwd_bar):
        fails.append(f"forward: worst row gap {np.nanmax(gap):.3e} > {fwd_bar:.3e} (row {int(np.nanargmax(gap))})")
    if not np.all(np.isfinite(z)):
        fails.append("forward: non-finite output")
    ok = ~ref.kink[:B]
    if np.count_nonzero(~ok) > kink_cap(B):
        fails.append(f"{np.count_nonzero(~ok)} kink rows of {B}: over the cap {kink_cap(B)}")
    ggap = row_gap(grad_q, ref.grad_q[:B])[ok]
    if ggap.size and not np.all(ggap <= bwd_bar):
        fails.append(f"backward: worst row gap {np.nanmax(ggap):.3e} > {bwd_bar:.3e}")
    inside = ref.interior[:B]
    if not np.all(iters[inside] == 0):
        fails.append("an interior row took iterations")
    if not np.array_equal(z[inside], ref.q[:B][inside]):
        fails.append("an interior row moved")
    if np.any(iters[~inside] == 0):
        fails.append("a row outside the set took no iteration")
    viol = float(np.max(cs.getViolationRows(z @ cs.NA_E.T + cs.yp.T)))
    if not viol <= viol_bar:
        fails.append(f"violation {viol:.3e} > {viol_bar:.3e}")
    return fails
