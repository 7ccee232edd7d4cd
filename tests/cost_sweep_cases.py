"""Cases of the soft-cost sweep (tests/test_gpu_soft_cost_sweep.py on the device, tests/test_soft_cost_sweep_host.py on the
host): every kernel instantiation, both sides of every cut-over, the tile and id book-keeping, exact cases and the limits.

The sets are hand-made ``set_arrays``-style dicts (``ops.CostPack`` and ``cost_reference.reference`` take nothing else): no
``ConvexConstraints``, no feasibility requirement.  Everything is seeded; the fp64 reference of a case is computed once."""
import functools

import numpy as np

import cost_cases
import cost_reference

LDS_BUDGET = 160 * 1024       # kLdsBudget of rayen_cost.hip


class SweepCase:
    """What helpers.cost_check / helpers.cost_device_y read of a case."""

    def __init__(self, name, arrays, y, pad=0, kind="mixed"):
        self.name, self.arrays, self.y, self.pad, self.kind = name, arrays, np.ascontiguousarray(y, dtype=np.float64), pad, kind
        self.ref = cost_reference.reference(arrays, self.y)
        self.y.setflags(write=False)

    def head(self, B):
        """The case of the first ``B`` rows."""
        return SweepCase(f"{self.name}[:{B}]", self.arrays, self.y[:B].copy(), self.pad, self.kind)


def make_set(k, A1=None, b1=None, quads=(), cones=(), A2=None, b2=None):
    """A ``soft_cost.set_arrays``-style dict from plain data; ``quads``: (P, q, r), ``cones``: (M, s, c, d)."""
    f = lambda a, *shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(*shape))          # noqa: E731
    out = dict(k=int(k))
    out["A1"] = f(A1, -1, k) if A1 is not None and len(A1) else np.zeros((0, k))
    out["b1"] = f(b1, -1) if b1 is not None and len(b1) else np.zeros(0)
    out["A2"] = f(A2, -1, k) if A2 is not None and len(A2) else np.zeros((0, k))
    out["b2"] = f(b2, -1) if b2 is not None and len(b2) else np.zeros(0)
    out["P"] = f([P for P, _, _ in quads], -1, k, k) if quads else np.zeros((0, k, k))
    out["q"] = f([q for _, q, _ in quads], -1, k) if quads else np.zeros((0, k))
    out["r"] = f([r for _, _, r in quads], -1) if quads else np.zeros(0)
    out["M"] = f(np.concatenate([np.reshape(M, (-1, k)) for M, _, _, _ in cones], axis=0), -1, k) if cones else np.zeros((0, k))
    out["s"] = f(np.concatenate([np.reshape(s, -1) for _, s, _, _ in cones]), -1) if cones else np.zeros(0)
    out["c"] = f([c for _, _, c, _ in cones], -1, k) if cones else np.zeros((0, k))
    out["d"] = f([d for _, _, _, d in cones], -1) if cones else np.zeros(0)
    out["soc_rows"] = np.asarray([np.reshape(M, (-1, k)).shape[0] for M, _, _, _ in cones], dtype=np.int32)
    out["F"] = np.zeros((0, 0, 0))
    assert out["A1"].shape[0] == out["b1"].size and out["A2"].shape[0] == out["b2"].size
    assert out["M"].shape[0] == out["s"].size == int(out["soc_rows"].sum())
    return out


def n_values(a):
    return a["b1"].size + a["r"].size + a["soc_rows"].size + a["b2"].size


def random_set(k, m1, nq, cone_rows, m2, seed):
    """Rows of unit scale around the origin (which is strictly inside every inequality)."""
    rng = np.random.default_rng(seed)
    quads, cones = [], []
    for _ in range(nq):
        G = rng.standard_normal((k, k)) / np.sqrt(k)
        quads.append((G @ G.T, 0.3 * rng.standard_normal(k), -rng.uniform(0.5, 1.5)))
    for rows in cone_rows:
        s = 0.3 * rng.standard_normal(rows) / np.sqrt(rows)
        cones.append((rng.standard_normal((rows, k)) / np.sqrt(k), s, 0.3 * rng.standard_normal(k),
                      np.linalg.norm(s) + rng.uniform(0.3, 0.8)))
    return make_set(k, rng.standard_normal((m1, k)) / np.sqrt(k), rng.uniform(0.5, 1.5, size=m1), quads, cones,
                    rng.standard_normal((m2, k)) / np.sqrt(k), 0.3 * rng.standard_normal(m2))


def random_rows(k, B, seed):
    """Rows from well inside to well outside."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=(B, k)) * rng.choice([0.05, 0.7, 3.0], size=(B, 1)) * np.sqrt(k)


# ------------------------------------------------------------------------------------------------------------------
# 1 width sweep (and 2 alignment, 7 NaN placement, 9 optional outputs, which reuse its sets)
# ------------------------------------------------------------------------------------------------------------------

WIDTHS = (1, 4, 8, 9, 16, 17, 32, 33, 36, 60, 63, 64)
WIDTH_B = 65


def lane64_K(k):
    """The fp64 kernel's register width for k columns (build64)."""
    return 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64


@functools.lru_cache(maxsize=None)
def width_case(k):
    """5 linear rows, 1 quadratic, one cone of 3 rows, 1 equality; 65 rows."""
    return SweepCase(f"width_k{k}", random_set(k, 5, 1, (3,), 1, seed=100 + k), random_rows(k, WIDTH_B, seed=200 + k))


ALIGN_WIDTHS = {"float32": (8, 36, 64), "float64": (8,)}
LAYOUTS = ("aligned", "offset1", "ld_k1")      # 16-byte rows | base one element past a 16-byte boundary | row stride k + 1


def layout(kind, k):
    """(elements between the 16-byte boundary and the first row, row stride) of a y / grad buffer."""
    ld4 = (k + 7) // 4 * 4          # a multiple of 4 with at least four padding columns
    return {"aligned": (0, ld4), "offset1": (1, ld4), "ld_k1": (0, k + 1)}[kind]


NAN_K, NAN_COLS, NAN_ROWS = 36, (0, 5, 33, 35), (0, 31, 32, 64)


def nan_case(col, row):
    base = width_case(NAN_K)
    y = base.y.copy()
    y[row, col] = np.nan
    return SweepCase(f"nan_c{col}_r{row}", base.arrays, y, kind="nan")


# ------------------------------------------------------------------------------------------------------------------
# 3 row tiles (k = 12, B = 65), 4 every index reportable
# ------------------------------------------------------------------------------------------------------------------

TILE_K, TILE_B = 12, 65
# name -> (m1, nq, cone rows, m2)
TILE_SETS = {
    "mixed": (33, 3, (33, 5, 64), 33),           # two linear tiles, three quadratics, cones of 2 / 1 / 2 tiles, two equality tiles
    "cone1": (0, 0, (1,), 0),
    "one_each": (1, 1, (31,), 1),
    "edge32": (31, 0, (32,), 32),
    "lin32_cone63": (32, 0, (63,), 0),
    "three_tiles": (65, 1, (64, 1), 65),
    "no_lin": (0, 3, (33, 32), 33),              # an equality tile after cones, no linear tile before
    "eq_only": (0, 0, (), 65),
    "cone_walk": (32, 1, (31, 33, 1), 1),        # one-tile, two-tile, one-tile: the t += ntile walk
    "lin_only": (33, 0, (), 0),
    "quad_only": (0, 1, (), 0),
    "cone65": (5, 0, (65,), 1),                  # fp32 refuses (a cone's products are held in two tiles), fp64 serves
}
TILE_REFUSED32 = ("cone65",)


def _mixed_set():
    """The ``mixed`` shape with rows scaled so that none is dominated: unit linear and equality rows, weak quadratics along
    directions of their own (they win far out), cones led by their linear part ``-c'y``."""
    k, (m1, nq, cone_rows, m2) = TILE_K, TILE_SETS["mixed"]
    rng = np.random.default_rng(31)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)          # noqa: E731
    quads, cones = [], []
    for _ in range(nq):
        v, G = unit(rng.standard_normal(k)), rng.standard_normal((k, k)) / np.sqrt(k)
        quads.append((0.02 * np.outer(v, v) + 0.001 * G @ G.T, 0.01 * rng.standard_normal(k), -rng.uniform(0.5, 1.5)))
    for rows in cone_rows:
        s = 0.3 * rng.standard_normal(rows) / np.sqrt(rows)
        cones.append((0.1 * rng.standard_normal((rows, k)) / np.sqrt(k), s, 1.3 * unit(rng.standard_normal(k)),
                      np.linalg.norm(s) + rng.uniform(0.3, 0.8)))
    return make_set(k, unit(rng.standard_normal((m1, k))), rng.uniform(0.5, 1.5, size=m1), quads, cones,
                    unit(rng.standard_normal((m2, k))), 0.3 * rng.standard_normal(m2))


@functools.lru_cache(maxsize=None)
def tile_set(name):
    if name == "mixed":
        return _mixed_set()
    m1, nq, cone_rows, m2 = TILE_SETS[name]
    return random_set(TILE_K, m1, nq, cone_rows, m2, seed=300 + sorted(TILE_SETS).index(name))


@functools.lru_cache(maxsize=None)
def tile_case(name):
    return SweepCase(f"tile_{name}", tile_set(name), random_rows(TILE_K, TILE_B, seed=400 + sorted(TILE_SETS).index(name)))


def _candidates(a, seed, center):
    """Seeded candidate rows around ``center``: along +- every stored row, every cone's ``c`` and every quadratic's leading
    direction at a geometric ladder of lengths (a face is the worst value just outside it, a quadratic far out), and random
    rows."""
    rng = np.random.default_rng(seed)
    k = a["k"]
    dirs = [a["A1"], a["A2"], -a["A2"], -a["c"], a["M"], -a["M"]]
    for P in a["P"]:
        w, V = np.linalg.eigh(0.5 * (P + P.T))
        dirs += [V[:, -1:].T, -V[:, -1:].T]
    dirs = np.concatenate([d for d in dirs if d.size], axis=0)
    dirs = dirs / np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-300)
    rows = [t * dirs for t in np.geomspace(0.02, 4000.0, 36)]
    rows += [s * rng.standard_normal((512, k)) for s in (0.3, 1.0, 3.0, 10.0)]
    return center + np.concatenate(rows, axis=0)


def _search_values(a, y):
    """The stacked values of one row ``y``, vectorised: what the SEARCH below steers by (what it finds is judged by the
    reference)."""
    Ps = 0.5 * (a["P"] + np.transpose(a["P"], (0, 2, 1)))
    u = a["M"] @ y + a["s"]
    ends = np.cumsum(a["soc_rows"])
    norms = np.array([np.linalg.norm(u[e - r:e]) for e, r in zip(ends, a["soc_rows"])])
    return np.concatenate((a["A1"] @ y - a["b1"], 0.5 * np.einsum("i,qij,j->q", y, Ps, y) + a["q"] @ y + a["r"],
                           norms - a["c"] @ y - a["d"], np.abs(a["A2"] @ y - a["b2"])))


def best_margin(a, j, start):
    """``(y, margin)`` maximising value j minus the largest other value, from ``start`` (SLSQP on the epigraph form).  For a
    linear or an equality-free row j this is a concave programme -- a linear function minus a maximum of convex ones -- so
    the optimum found is the global one: a negative margin proves that index j is never the worst value."""
    from scipy.optimize import minimize
    k = a["k"]
    values = lambda y: _search_values(a, y)          # noqa: E731
    res = minimize(lambda x: -x[k], np.concatenate((np.reshape(start, -1), [-1.0])), method="SLSQP",
                   constraints=[dict(type="ineq", fun=lambda x: np.delete(values(x[:k])[j] - values(x[:k]), j) - x[k])],
                   options=dict(maxiter=300))
    v = cost_reference.reference(a, res.x[None, :k])["vals"][0]
    return res.x[:k], float(v[j] - np.max(np.delete(v, j)))


COVERAGE = ("mixed", "k17_m33")
# stacked indices that are never the worst value (the host test proves it with best_margin)
COVERAGE_UNREACHABLE = {"mixed": (), "k17_m33": (6, 32)}


def _coverage_rows(a, seed, center, skip=()):
    """One row per stacked index at which that index is the decided worst at the fp32 bars: the best-separated of the seeded
    candidates, and for an index no candidate reaches the maximiser of its margin."""
    y = _candidates(a, seed, center)
    found = cost_reference.reference(a, y)["which"]
    extra = [best_margin(a, j, center)[0] for j in range(n_values(a)) if j not in skip and not np.any(found == j)]
    y = np.concatenate([y] + [e[None] for e in extra], axis=0).astype(np.float32).astype(np.float64)      # (fp32 reads these, too)
    ref = cost_reference.reference(a, y)
    dvals = cost_reference.bounds(ref, 2.0 ** -24)[0]
    decided = cost_reference.which_is_decided(ref, dvals)
    v = np.sort(ref["vals"], axis=1)
    margin = (v[:, -1] - v[:, -2]) / np.maximum(np.max(dvals, axis=1), 1e-300)
    picked = []
    for j in range(n_values(a)):
        rows = np.flatnonzero(decided & (ref["which"] == j))
        if rows.size:
            picked.append(rows[np.argmax(margin[rows])])
    return y[picked], ref["which"][picked]


@functools.lru_cache(maxsize=None)
def coverage_case(name):
    if name == "mixed":
        arrays, center = tile_set("mixed"), np.zeros((1, TILE_K))
    else:
        base = cost_cases.case("k17_m33")
        arrays, center = base.arrays, np.asarray(base.cs.y0, dtype=np.float64).reshape(1, -1)
    y, _ = _coverage_rows(arrays, 500 + len(name), center, COVERAGE_UNREACHABLE[name])
    return SweepCase(f"coverage_{name}", arrays, y)


# ------------------------------------------------------------------------------------------------------------------
# 5 batch geometry
# ------------------------------------------------------------------------------------------------------------------

BATCHES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)


@functools.lru_cache(maxsize=None)
def batch_case():
    """257 rows against the ``quad_soc7`` set (k = 7)."""
    base = cost_cases.case("quad_soc7")
    y0 = np.asarray(base.cs.y0, dtype=np.float64).reshape(1, -1)
    rng = np.random.default_rng(77)
    span = 1.0 + float(np.max(np.abs(y0)))
    y = y0 + span * rng.uniform(-1.0, 1.0, size=(257, base.cs.k)) * rng.choice([0.02, 0.3, 1.5], size=(257, 1))
    return SweepCase("batch_quad_soc7", base.arrays, y)


def rounds_batch(cus, dtype_name):
    """The smallest interesting batch whose persistent loop takes a second round: fp32 deals groups of 32 rows over 4 waves per
    CU, fp64 blocks of 256 rows over the CUs."""
    return 128 * cus + 33 if dtype_name == "float32" else 256 * cus + 257


@functools.lru_cache(maxsize=None)
def rounds_case(B):
    base = cost_cases.case("lin5_eq2")
    y0 = np.asarray(base.cs.y0, dtype=np.float64).reshape(1, -1)
    rng = np.random.default_rng(B)
    span = 1.0 + float(np.max(np.abs(y0)))
    y = y0 + span * rng.uniform(-1.0, 1.0, size=(B, base.cs.k)) * rng.choice([0.02, 0.3, 1.5], size=(B, 1))
    return SweepCase(f"rounds_{B}", base.arrays, y)


# ------------------------------------------------------------------------------------------------------------------
# 6 exact cases: small integers, so every product and sum is exact in fp32 and the assertions are equalities
# ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tie_case():
    """41 linear rows and one equality row, k = 4.  Rows 1 and 5 are the same row (the two lane halves of a tile), rows 2 and
    40 are the same row (two tiles), and the equality row 41 repeats row 3.  Every other row sits 100 below."""
    k, m1 = 4, 41
    rng = np.random.default_rng(61)
    A1 = rng.integers(-1, 2, size=(m1, k)).astype(np.float64)
    b1 = np.full(m1, 100.0)
    for rows, col in (((1, 5), 0), ((2, 40), 1), ((3,), 2)):
        for r in rows:
            A1[r], b1[r] = np.eye(k)[col], 0.0
    y = rng.integers(-8, 9, size=(64, k)).astype(np.float64)
    y[:6] = [[5, 1, 1, 0], [1, 6, 2, 0], [1, 2, 7, 0], [3, 3, 3, 0], [-1, -1, -4, 0], [0, -1, -2, 0]]
    return SweepCase("exact_ties", make_set(k, A1, b1, A2=np.eye(k)[2:3], b2=[0.0]), y)


# (sample, the lowest index among the tied largest values, every index that ties)
TIES = ((0, 1, (1, 5)), (1, 2, (2, 40)), (2, 3, (3, 41)), (3, 1, (1, 2, 3, 5, 40, 41)))


@functools.lru_cache(maxsize=None)
def zero_case():
    """Rows whose largest value is exactly 0 (relu on its kink): the cost, the worst value and the whole gradient are 0."""
    k = 4
    A1 = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, -1]], dtype=np.float64)
    b1 = np.array([2.0, 3.0, 6.0, 1.0])
    quad = (2.0 * np.eye(k), np.zeros(k), -1250.0)                   # y'y - 1250
    cone = (np.eye(k)[:2], np.zeros(2), np.array([0, 0, 0, 1.0]), 20.0)
    y = np.array([[2, 1, 0, 0], [0, 3, 0, 0], [1, 3, 0, 0], [-3, -4, 1, 0],          # a linear row at 0
                  [0, 0, 25, 25], [-3, -4, -30, -15],                                # the quadratic | the cone (norm 5) at 0
                  [2, 3, 26, 25], [3, 3, 0, 0]], dtype=np.float64)                   # violated: the quadratic | linear rows
    return SweepCase("exact_zero", make_set(k, A1, b1, [quad], [cone]), y)


ZERO_ROWS = (0, 1, 2, 3, 4, 5)          # samples of zero_case whose largest value is exactly 0 (the others violate)


@functools.lru_cache(maxsize=None)
def apex_case():
    """A cone of 2 rows in 4 columns, s = 0: rows with y in the null space of M sit on the apex (||My + s|| == 0) with
    ``g = -c'y - d > 0``, where the gradient is exactly ``-2 g c``.  Two further rows have ``||My|| = 5`` (3-4-5)."""
    k = 4
    cone = (np.eye(k)[:2], np.zeros(2), np.array([0, 0, 1.0, 2.0]), 1.0)
    y = np.array([[0, 0, -2, -3], [0, 0, -3, 0], [0, 0, -40, 7], [0, 0, 5, 5], [3, 4, -2, -3], [5, 0, 1, 1]], dtype=np.float64)
    return SweepCase("exact_apex", make_set(k, [[1, 1, 1, 1]], [1000.0], cones=[cone]), y)


APEX_ROWS = (0, 1, 2)             # violated on the apex; row 3 is on the apex and inside (g < 0)


@functools.lru_cache(maxsize=None)
def lone_lane_case():
    """65 rows of which only sample 17 violates anything, against 33 linear rows (two tiles) and a cone: the ballot-guarded
    coefficient products run for a wave in which one lane has a non-zero coefficient, and not at all for the other waves."""
    k, m1 = 4, 33
    rng = np.random.default_rng(62)
    A1 = rng.integers(-3, 4, size=(m1, k)).astype(np.float64)
    cone = (np.eye(k)[:2], np.zeros(2), np.array([0, 0, 1.0, 0]), 2.0)
    y = np.zeros((65, k))
    y[17] = [4, 0, -3, 2]          # (a norm of 4: the kernel's 2 relu(g) / norm is exact, too)
    y[40] = [0, 0, 1, 0]          # inside, not at the origin
    return SweepCase("exact_lone_lane", make_set(k, A1, np.full(m1, 4.0), cones=[cone]), y)


EXACT = {"ties": tie_case, "zero": zero_case, "apex": apex_case, "lone_lane": lone_lane_case}


def exact_premises(c):
    """True when every input is a small integer (quadratics: an even P) and every intermediate of cost, worst and gradient is
    an integer below 2^24 in magnitude -- so fp32 computes each exactly, in any order.  Cones are exempt from the integer
    premise on their norm: the callers assert equality only on rows where it is 0."""
    a, y = c.arrays, c.y
    ints = all(np.array_equal(x, np.round(x)) for x in (a["A1"], a["b1"], a["q"], a["r"], a["M"], a["s"], a["c"], a["d"],
                                                          a["A2"], a["b2"], y))
    ints = ints and np.array_equal(0.5 * a["P"], np.round(0.5 * a["P"]))
    S = c.ref["S"]
    cost_terms = np.sum(S * S, axis=1)
    grad_terms = sum(2.0 * S[:, j:j + 1] * np.maximum(np.abs(c.ref["dirs"][j]), 1.0) for j in range(S.shape[1]))
    # (a quadratic's direction P y + q is bounded by its own sum of absolute terms)
    return bool(ints and np.max(cost_terms) < 2.0 ** 24 and np.max(grad_terms) < 2.0 ** 24)


# ------------------------------------------------------------------------------------------------------------------
# 8 limits: the image bytes from the layout in RayenCostPack's comments
# ------------------------------------------------------------------------------------------------------------------

def image_bytes32(m1, nq, cone_rows, m2):
    """fp32 image, 4-byte words: W [nt][32][64] | rowc [nt][32] | colv [nf][64] | desc [nt][8], rounded up to 16 bytes.
    Linear and equality rows in tiles of 32, a quadratic in two tiles, a cone in one (<= 32 rows) or two."""
    nt = -(-m1 // 32) + 2 * nq + sum(2 if r > 32 else 1 for r in cone_rows) + -(-m2 // 32)
    nf = nq + len(cone_rows)
    return (4 * (nt * 2048 + nt * 32 + nf * 64 + nt * 8) + 15) // 16 * 16


def image_bytes64(m1, nq, cone_rows, m2, k):
    """fp64 image, 8-byte words: W [R][K] | rowc [R] | colv [nf][K] | fconst [ni] | desc [ni][8 ints], rounded up to 16
    bytes.  R stacks every row (a quadratic has k), one item per family member (all linear rows are one item)."""
    K = lane64_K(k)
    R, nf = m1 + nq * k + sum(cone_rows) + m2, nq + len(cone_rows)
    ni = (m1 > 0) + nq + len(cone_rows) + (m2 > 0)
    return (8 * (R * K + R + nf * K + ni + ni * 4) + 15) // 16 * 16


def served_by_formula(a, dtype_name):
    rows = [int(r) for r in a["soc_rows"]]
    if a["k"] > 64:
        return False
    if dtype_name == "float32":
        return max(rows, default=0) <= 64 and image_bytes32(a["b1"].size, a["r"].size, rows, a["b2"].size) <= LDS_BUDGET
    return image_bytes64(a["b1"].size, a["r"].size, rows, a["b2"].size, a["k"]) <= LDS_BUDGET


LIMIT_K = 8


def limit_rows(dtype_name):
    """The largest linear-only set (k = 8) whose image the precision serves."""
    m = 1
    while (image_bytes32(m + 1, 0, (), 0) if dtype_name == "float32" else image_bytes64(m + 1, 0, (), 0, LIMIT_K)) <= LDS_BUDGET:
        m += 1
    return m


@functools.lru_cache(maxsize=None)
def limit_case(m1):
    rng = np.random.default_rng(m1)
    k = LIMIT_K
    return SweepCase(f"limit_m{m1}", make_set(k, rng.standard_normal((m1, k)) / np.sqrt(k), rng.uniform(0.5, 1.5, size=m1)),
                     random_rows(k, 65, seed=m1 + 1))


@functools.lru_cache(maxsize=None)
def k65_case():
    return SweepCase("k65", random_set(65, 3, 0, (), 1, seed=65), random_rows(65, 4, seed=66))


NOMINAL_CUS = 256          # the host test's stand-in for the device's CU count (the GPU test asks the device)


def all_cases():
    """name -> builder of every case of the sweep (the host test runs the mirror on each)."""
    out = {f"width_k{k}": functools.partial(width_case, k) for k in WIDTHS}
    out.update({f"nan_c{c}_r{r}": functools.partial(nan_case, c, r) for c in NAN_COLS for r in NAN_ROWS})
    out.update({f"tile_{n}": functools.partial(tile_case, n) for n in TILE_SETS})
    out.update({f"coverage_{n}": functools.partial(coverage_case, n) for n in COVERAGE})
    out["batch_quad_soc7"] = batch_case
    out.update({f"rounds_{d}": functools.partial(rounds_case, rounds_batch(NOMINAL_CUS, d)) for d in ("float32", "float64")})
    out.update({f"exact_{n}": fn for n, fn in EXACT.items()})
    out.update({f"limit_{d}": (lambda d=d: limit_case(limit_rows(d))) for d in ("float32", "float64")})
    return out


INF_ROWS = (7, 40)


@functools.lru_cache(maxsize=None)
def inf_case():
    """Two cones (33 rows: two tiles with one valid row in the second; 5 rows) in 12 columns, and +inf in column 3 of two
    samples, where both ``c`` are negative: every valid row of ``My + s`` is infinite, so the value is ``inf - (-inf) = inf``
    and the cost is inf, not NaN -- unless a zero padding row of a tile (0 x inf = NaN) gets into the norm."""
    a = random_set(TILE_K, 0, 0, (33, 5), 0, seed=71)
    a["c"][:, 3] = -np.abs(a["c"][:, 3]) - 0.1
    assert np.all(a["M"][:, 3] != 0)
    y = random_rows(TILE_K, 65, seed=72)
    y[list(INF_ROWS), 3] = np.inf
    return y, a
