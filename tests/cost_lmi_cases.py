"""Seeded cases, fp64 reference and bars of the soft cost of sets WITH an LMI (rayen_amd/csrc/rayen_cost_lmi.hip), shared by
tests/test_cost_lmi_reference_host.py and tests/test_gpu_soft_cost_lmi.py.

Reference (:func:`reference`): numpy ``eigh`` in fp64, one sample at a time.  ``g = -lambda_min(F(y))``, the LMI's gradient
``2 relu(g) dg/dy_a`` with ``dg/dy_a = -x'F_a x`` from the eigenvector ``x`` of ``lambda_min``; the set's other rows come from
tests/cost_reference.py and everything is put in the stacked order ``lin_ineq, quad, soc, lmi, lin_eq``.  Per sample also
``scale = max(||F(y)||_inf, 1)`` (row-sum norm: the size the LMI's value is measured against) and ``gap = (lambda_1 -
lambda_0) / ||F(y)||_2``, the gap between the two smallest eigenvalues relative to the spectral norm -- the quantity the
eigenvector's condition ``r eps ||F|| / (lambda_1 - lambda_0)`` is written in.

Sets.  The generators are dense, with a planted spectrum so that the eigenvector is well conditioned on most rows (a plain
random ``T T' + I / 2`` offset has its smallest eigenvalues in a cluster: no interior row would pass the gap condition):
``F_k = Q diag(0.5, 1, 3, 2.2, 1.2 .. 1.6) Q'``, ``F_a = W_a / ||W_a|| - 3 u_a u_a'`` (``W_a`` uniform symmetric, ``u_a`` a
random unit vector) and ``F_0 = ALPHA I - F_k``, so that ``y = e_0`` gives ``F(y) = ALPHA I``: the fully degenerate row,
outside the set (``g = -ALPHA > 0``), exact in fp32 off the diagonal.

Rows of a batch of 67 (:func:`_kinds`): interior (``g`` far below 0), far outside (2 to 4 times the ray's exit), rows scaled along a ray so that ``g`` is
``+-{1/2, 1, 2}`` times 1e-5 or 1e-9 of the scale (the sizes of the fp32 and the fp64 bar), one degenerate row, one NaN row.
Batches of 1 and 3 are the first rows of ``outside, degenerate, NaN``.

Gradient rows: only rows with ``gap >= 1e-2`` are held to the gradient bar (``kept``); the degenerate row is exempt (it has
bars of its own).  This uses the fp64 reference alone and is the only exclusion; at least three quarters of a batch's finite
rows are kept (asserted here).

Bars (:func:`check`), ``d`` being the bar of the LMI's value per row:
  * fp64 ``d = 1e-9 scale``; fp32 ``d = max(1e-5 scale, 2 |LAPACK fp32 eigvalsh - fp64 truth|)`` on the same row
    (the bar of tests/test_gpu_lmi_wave.py for the same device helpers);
  * ``cost``: ``2 |g| d + d^2`` (``relu`` is 1-Lipschitz), plus the rows' own bar of tests/cost_reference.py on a mixed set;
  * ``worst``: the largest bar among the row's values; ``which`` wherever the two largest values are further apart than
    their bars;
  * gradient of the LMI on kept rows: ``max(tol, 8 r eps / gap) * max_a |ref_a|`` with tol 2e-3 / eps 6e-8 (fp32) and 1e-7 /
    1.1e-16 (fp64), the constants of tests/test_gpu_lmi_wave.py:68-72, PLUS ``2 d ||F_a||_2``.  The second term is the error
    of the factor ``2 relu(g)`` itself: the gradient is ``2 relu(g) w`` with ``|w_a| <= ||F_a||_2``, and an answer whose
    ``g`` is off by its bar ``d`` moves it by up to ``2 d |w_a|`` -- for the rows placed AT the bar that is as large as the
    gradient (the reference's gradient is exactly 0 one bar inside), so a purely relative bound cannot hold for them in any
    arithmetic; where ``g >> d`` the term is below the relative one.  A row with ``g < -d`` must answer exactly 0;
  * degenerate row: values at the bars above, a finite gradient with ``|grad_a| <= 2 relu(g) ||F_a||_2 (1 + 1e-3)``;
  * NaN row: ``cost = worst = NaN``, ``which = -1``.
"""
import functools

import numpy as np

from rayen_amd import workloads
from rayen_amd.soft_cost import set_arrays

import cost_cases
import cost_reference

ALPHA = -0.7
LDS_LIMIT_BYTES = 150 * 1024          # include/rayen_hip.h: r (r | 1) + 6 r + 3 k + 10 elements within 150 KiB


def lds_elems(k, r):
    return r * (r | 1) + 6 * r + 3 * k + 10


def r_max(k, itemsize):
    r = 1
    while lds_elems(k, r + 1) * itemsize <= LDS_LIMIT_BYTES:
        r += 1
    return r


R_MAX32, R_MAX64 = r_max(5, 4), r_max(5, 8)          # 192, 135

# name -> (k, r, rows of the set besides the LMI)
SETS = {
    "k1_r1": (1, 1, None), "k3_r2": (3, 2, None), "k4_r3": (4, 3, None), "k10_r20": (10, 20, None),
    "k6_r63": (6, 63, None), "k6_r64": (6, 64, None), "k6_r65": (6, 65, None),
    "k70_r12": (70, 12, None),                         # k beyond the matrix-core kernel's 64 columns
    "k5_rmax32": (5, R_MAX32, None), "k5_rmax64": (5, R_MAX64, None),
    "k5_over32": (5, R_MAX32 + 1, None), "k5_over64": (5, R_MAX64 + 1, None),      # refused (over64: in fp64 only)
    "lin5_eq2_lmi8": (6, 8, "lin5_eq2"),               # 5 linear rows + 2 equalities + an 8 x 8 LMI
    "quad_soc7_lmi5": (7, 5, "quad_soc7"),             # quad_soc7 of tests/cost_cases.py + a 5 x 5 LMI
}
SERVED = tuple(n for n in SETS if "over" not in n)
MIXED = ("lin5_eq2_lmi8", "quad_soc7_lmi5")
BATCHES = (1, 3, 67)
TOL = {"float32": (2e-3, 6e-8), "float64": (1e-7, 1.1e-16)}
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}


def served(name, dtype_name):
    k, r, _ = SETS[name]
    return lds_elems(k, r) * (4 if dtype_name == "float32" else 8) <= LDS_LIMIT_BYTES


def generators(k, r, seed):
    """``F [k + 1, r, r]`` (constant term last), module docstring."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((r, r)))
    lam = np.array([0.5, 1.0, 3.0, 2.2] + list(np.linspace(1.2, 1.6, max(r - 4, 0))))[:r]
    Fk = (Q * lam) @ Q.T
    Fk = 0.5 * (Fk + Fk.T)
    F = [ALPHA * np.eye(r) - Fk]
    for _ in range(1, k):
        T = rng.uniform(-1.0, 1.0, size=(r, r))
        W = 0.5 * (T + T.T)
        u = rng.standard_normal(r)
        u /= np.linalg.norm(u)
        F.append(W / max(np.linalg.norm(W, 2), 1e-300) - 3.0 * np.outer(u, u))
    return F + [Fk]


def _raw(name):
    k, r, rows = SETS[name]
    seed = sum(map(ord, name))
    if rows is None:
        raw = workloads._empty(k)
    elif rows == "lin5_eq2":
        rng = np.random.default_rng(seed)
        raw = workloads._empty(k)
        raw["A1"], raw["b1"] = rng.uniform(-1.0, 1.0, size=(5, k)), rng.uniform(0.1, 1.0, size=(5, 1))
        raw["A2"], raw["b2"] = rng.uniform(-1.0, 1.0, size=(2, k)), np.zeros((2, 1))          # y0 = 0 satisfies them
    else:
        raw = cost_cases._raws()[rows]
    assert raw["y0"].shape[0] == k and not np.any(raw["y0"])
    raw["F"] = generators(k, r, seed)
    return raw


@functools.lru_cache(maxsize=None)
def the_set(name):
    """``(cs, arrays, arrays of the set without its LMI | None, arrays of the LMI alone)``."""
    cs = workloads.build_constraints(_raw(name))
    arrays = set_arrays(cs)
    rows = dict(arrays, F=np.zeros((0, 0, 0))) if SETS[name][2] else None
    alone = dict(arrays, F=arrays["F"])
    for key in ("A1", "P", "q", "M", "c", "A2"):
        alone[key] = arrays[key][:0]
    for key in ("b1", "r", "s", "d", "soc_rows", "b2"):
        alone[key] = arrays[key][:0]
    return cs, arrays, rows, alone


def lmi_reference(F, y):
    """Per sample: ``g``, ``x`` (eigenvector of lambda_min), ``w [B, k]`` (``dg/dy``), ``scale``, ``gap``; NaN rows NaN."""
    B, k = y.shape
    r = F.shape[1]
    g, scale, gap = np.full(B, np.nan), np.full(B, np.nan), np.full(B, np.nan)
    w, lam_max = np.full((B, k), np.nan), np.full(B, np.nan)
    for b in range(B):
        if not np.all(np.isfinite(y[b])):
            continue
        H = F[-1] + np.tensordot(y[b], F[:-1], axes=1)
        lam, V = np.linalg.eigh(H)
        x = V[:, 0]
        g[b] = -lam[0]
        lam_max[b] = lam[-1]
        scale[b] = max(float(np.max(np.sum(np.abs(H), axis=1))), 1.0)
        gap[b] = (lam[1] - lam[0]) / max(float(np.max(np.abs(lam))), 1e-300) if r > 1 else np.inf
        w[b] = -np.einsum("i,aij,j->a", x, F[:-1], x)
    return dict(g=g, w=w, scale=scale, gap=gap, lam_max=lam_max)


def reference(arrays, y):
    """The whole set: ``cost, worst, which, grad`` per sample, every value ``vals [B, n]`` in the stacked order, the LMI's part
    (``lmi``: :func:`lmi_reference`, ``lmi_cost``, ``lmi_grad``), the rows' part (``rows``: cost_reference.reference | None)
    and ``lmi_id``."""
    y = np.asarray(y, dtype=np.float64)
    B = y.shape[0]
    n_eq = int(arrays["b2"].size)
    has_rows = int(arrays["b1"].size + arrays["r"].size + arrays["soc_rows"].size) + n_eq > 0
    rows = cost_reference.reference(arrays, y) if has_rows else None
    lmi = lmi_reference(arrays["F"], y)
    p = np.where(lmi["g"] < 0, 0.0, lmi["g"])                      # relu that keeps a NaN
    lmi_cost, lmi_grad = p * p, 2.0 * p[:, None] * lmi["w"]
    if rows is None:
        vals, cost, grad, lmi_id = lmi["g"][:, None], lmi_cost, lmi_grad, 0
    else:
        lmi_id = rows["vals"].shape[1] - n_eq
        vals = np.concatenate((rows["vals"][:, :lmi_id], lmi["g"][:, None], rows["vals"][:, lmi_id:]), axis=1)
        cost, grad = rows["cost"] + lmi_cost, rows["grad"] + lmi_grad
    bad = np.isnan(cost)
    safe = np.where(bad[:, None], 0.0, vals)
    which = np.where(bad, -1, np.argmax(safe, axis=1)).astype(np.int32)
    worst = np.where(bad, np.nan, np.max(safe, axis=1))
    grad = np.where(bad[:, None], np.nan, grad)
    return dict(cost=cost, worst=worst, which=which, grad=grad, vals=vals, lmi=lmi, lmi_cost=lmi_cost, lmi_grad=lmi_grad,
                rows=rows, lmi_id=lmi_id, n_eq=n_eq)


# ---------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------

def _kinds(B):
    if B <= 3:
        return ["outside", "degenerate", "nan"][:B]
    kinds = ["interior"] * 12 + ["outside"] * 24 + ["near"] * 24 + ["mid"] * (B - 60)
    kinds[33], kinds[40] = "nan", "degenerate"
    return kinds


def _exit(F, direction):
    """``t0 > 0`` at which the ray ``t direction`` leaves the LMI (``F_k + t D`` singular), or None when it never does."""
    D = np.tensordot(direction, F[:-1], axes=1)
    Li = np.linalg.inv(np.linalg.cholesky(F[-1]))
    mu = np.linalg.eigvalsh(Li @ D @ Li.T)[0]
    return None if mu >= -1e-12 else -1.0 / mu


def _on_ray(F, direction, fraction):
    """``t direction`` with ``g = fraction * scale`` to first order around the point where the ray leaves the LMI (``g`` is
    convex along the ray and negative at 0), or None when it never leaves."""
    t0 = _exit(F, direction)
    if t0 is None:
        return None
    D = np.tensordot(direction, F[:-1], axes=1)
    H = F[-1] + t0 * D
    lam, V = np.linalg.eigh(H)
    slope = -float(V[:, 0] @ D @ V[:, 0])              # dg/dt > 0
    scale = max(float(np.max(np.sum(np.abs(H), axis=1))), 1.0)
    return (t0 + fraction * scale / slope) * direction


class Case:
    def __init__(self, name, B):
        self.name, self.B = name, B
        self.cs, self.arrays, self.rows_arrays, self.alone_arrays = the_set(name)
        self.k, self.r, _ = SETS[name]
        self.kinds = _kinds(B)
        F = self.arrays["F"]
        rng = np.random.default_rng(1000 * B + sum(map(ord, name)))
        y = np.zeros((B, self.k))
        steps = [s * m for m in (1e-5, 1e-9) for s in (0.5, -0.5, 1.0, -1.0, 2.0, -2.0)]
        for b, kind in enumerate(self.kinds):
            u = rng.uniform(-1.0, 1.0, size=self.k)
            if kind == "interior":
                y[b] = 0.02 * u
            elif kind == "outside":              # two to four times as far as where the ray leaves the set
                t0 = _exit(F, u)
                if t0 is None:
                    u = -u
                    t0 = _exit(F, u)
                y[b] = rng.uniform(2.0, 4.0) * (1.0 if t0 is None else t0) * u
            elif kind == "mid":
                y[b] = 0.7 * u
            elif kind == "degenerate":
                y[b, 0] = 1.0
            elif kind == "near":
                at = _on_ray(F, u, steps[b % len(steps)])
                y[b] = u if at is None else at       # (a ray that never leaves the set: an interior row)
            else:
                y[b] = u
                y[b, self.k // 2] = np.nan
        self.y = y
        self.y.setflags(write=False)
        self.ref = reference(self.arrays, y)
        self.finite = ~np.isnan(self.ref["cost"])
        self.degenerate = np.array([kd == "degenerate" for kd in self.kinds])
        # the gradient rows: the only exclusion anywhere, from the fp64 reference alone
        self.kept = self.finite & ~self.degenerate & (self.ref["lmi"]["gap"] >= 1e-2)
        assert (self.kept | self.degenerate)[self.finite].sum() >= 0.75 * self.finite.sum(), (name, B)
        self.fnorm = np.array([np.linalg.norm(Fa, 2) for Fa in F[:-1]])

    def reference_for(self, dtype_name):
        """The reference on what a kernel of that precision reads (``y`` rounded to fp32), and LAPACK's fp32 ``g``."""
        if dtype_name == "float64":
            return self.ref, None
        if not hasattr(self, "_ref32"):
            y32 = self.y.astype(np.float32)
            ref = reference(self.arrays, y32.astype(np.float64))
            F32 = self.arrays["F"].astype(np.float32)
            g32 = np.full(self.B, np.nan)
            for b in np.flatnonzero(self.finite):
                H = F32[-1] + np.tensordot(y32[b], F32[:-1], axes=1)
                g32[b] = -float(np.linalg.eigvalsh(H.astype(np.float32))[0])
            self._ref32 = (ref, g32)
        return self._ref32


@functools.lru_cache(maxsize=None)
def case(name, B):
    return Case(name, B)


# ---------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------

def value_bar(c, dtype_name):
    """``d [B]``: the bar of the LMI's value (module docstring); ``(ref, d)``."""
    ref, g32 = c.reference_for(dtype_name)
    scale = ref["lmi"]["scale"]
    if dtype_name == "float64":
        return ref, 1e-9 * scale
    return ref, np.maximum(1e-5 * scale, 2.0 * np.abs(g32 - ref["lmi"]["g"]))


def check(c, dtype_name, cost, worst, which, grad, what):
    """``cost, worst, which [B]`` and ``grad [B, k] | None`` (arrays) of the whole set against the reference at the bars of
    the module docstring; an AssertionError names the first figure that misses."""
    ref, d = value_bar(c, dtype_name)
    u = U[dtype_name]
    cost, worst, which = (np.asarray(t) for t in (cost, worst, which))
    cost, worst = cost.astype(np.float64), worst.astype(np.float64)
    bad, ok = ~c.finite, c.finite
    g = ref["lmi"]["g"]
    assert np.array_equal(np.isnan(cost), bad) and np.array_equal(np.isnan(worst), bad), what + ": NaN rows"
    assert np.all(which[bad] == -1), what + ": which of a NaN row"
    dl = np.where(ok, d, 0.0)
    dcost = 2.0 * np.abs(np.where(ok, g, 0.0)) * dl + dl * dl
    dvals = dl[:, None]
    dgrad = None
    if ref["rows"] is not None:
        rvals, rcost, dgrad = cost_reference.bounds(ref["rows"], u)
        i = ref["lmi_id"]
        dvals = np.concatenate((rvals[:, :i], dl[:, None], rvals[:, i:]), axis=1)
        dcost = dcost + np.where(ok, rcost, 0.0)
    wtol = np.max(np.where(ok[:, None], dvals, 0.0), axis=1)
    print(f"{what}: worst gap/bar {np.max((np.abs(worst - ref['worst']) / np.maximum(wtol, 1e-300))[ok], initial=0.0):.3f} "
          f"cost gap/bar {np.max((np.abs(cost - ref['cost']) / np.maximum(dcost, 1e-300))[ok], initial=0.0):.3f}")
    assert np.all(np.abs(worst - ref["worst"])[ok] <= wtol[ok]), what + ": worst"
    assert np.all(np.abs(cost - ref["cost"])[ok] <= dcost[ok]), what + ": cost"
    # which: wherever the two largest values are further apart than their bars
    vals = np.where(ok[:, None], ref["vals"], -np.inf)
    rows = np.arange(c.B)
    if vals.shape[1] > 1:
        order = np.argsort(-vals, axis=1)
        top, second = order[:, 0], order[:, 1]
        with np.errstate(invalid="ignore"):
            sep = vals[rows, top] - vals[rows, second]
        others = np.where(np.arange(vals.shape[1])[None, :] == top[:, None], 0.0, dvals)
        decided = ok & (sep > dvals[rows, top] + np.max(others, axis=1))
    else:
        decided = ok
    assert np.array_equal(which[decided], ref["which"][decided]), what + ": which"
    assert np.all((which[ok] >= 0) & (which[ok] < vals.shape[1])), what + ": which out of range"
    if grad is None:
        return ref
    grad = np.asarray(grad).astype(np.float64)
    assert np.all(np.isfinite(grad[ok])), what + ": gradient not finite"
    tol, eps = TOL[dtype_name]
    gap = np.where(ok, ref["lmi"]["gap"], 1.0)
    rel = np.maximum(tol, 8.0 * c.r * eps / np.maximum(gap, 1e-300))
    size = np.max(np.abs(np.where(ok[:, None], ref["lmi_grad"], 0.0)), axis=1)
    bar = (rel * size)[:, None] + 2.0 * dl[:, None] * c.fnorm[None, :]
    if dgrad is not None:
        bar = bar + np.where(ok[:, None], dgrad, 0.0)
    err = np.abs(grad - ref["grad"])
    kept = c.kept
    print(f"{what}: grad gap/bar {np.max((err / np.maximum(bar, 1e-300))[kept], initial=0.0):.3f} on {int(kept.sum())} rows")
    assert np.all(err[kept] <= bar[kept]), what + ": gradient"
    # clearly inside (of the LMI): exactly nothing from it
    inside = ok & (g < -d)
    rows_grad = ref["rows"]["grad"] if ref["rows"] is not None else np.zeros_like(grad)
    if ref["rows"] is None:
        assert np.all(cost[inside] == 0.0) and np.all(grad[inside] == 0.0), what + ": interior rows"
    else:
        assert np.all(np.abs(grad - rows_grad)[inside] <= dgrad[inside]), what + ": interior rows"
    # the degenerate row: any unit vector is an eigenvector (on a mixed set the rows' part comes off, with its bar)
    for b in np.flatnonzero(c.degenerate & ok):
        lim = 2.0 * max(g[b], 0.0) * c.fnorm * (1.0 + 1e-3)
        slack = dgrad[b] if dgrad is not None else 0.0
        assert np.all(np.abs(grad[b] - rows_grad[b]) <= lim + slack), what + ": degenerate row"
    return ref
