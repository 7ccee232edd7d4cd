"""Cases of the streamed soft cost (rayen_amd/csrc/rayen_cost_stream.hip): the sets beyond the resident kernels' LDS limit,
the forced window sizes, and a Python restatement of the window partition of rayen_amd/csrc/rayen_cost_stream_layout.h
(tests/test_cost_stream_host.py holds the two against each other; tests/test_gpu_soft_cost_stream.py runs the cases).

The sets are ``set_arrays``-style dicts built with ``cost_sweep_cases.make_set`` / ``random_set`` (``ops.CostPack`` and
``cost_reference.reference`` take nothing else); everything is seeded and the fp64 reference of a case is computed once."""
import functools

import numpy as np

import cost_cases
import cost_lmi_cases as L
import cost_reference
import cost_sweep_cases as sweep

LDS_BUDGET = 160 * 1024                     # kLdsBudget
DEFAULT_WINDOW = LDS_BUDGET // 2            # kCostStreamWindow: two buffers, no other LDS
TILE_BYTES32 = 4 * (2048 + 32 + 8)          # a tile of W, its rowc and its descriptor
FORM_BYTES32 = 4 * 64
MIN_WINDOW32 = 2 * TILE_BYTES32 + FORM_BYTES32      # kCostStreamMinWindow32: a quadratic, or a cone of two tiles
DTYPES = ("float32", "float64")


# ------------------------------------------------------------------------------------------------------------------
# the partition, restated (closed forms where the header counts unit by unit)
# ------------------------------------------------------------------------------------------------------------------

def bytes32(nt, nf):
    return TILE_BYTES32 * nt + FORM_BYTES32 * nf


def bytes64(R, nf, ni, K):
    return (8 * (R * K + R + nf * K + ni + 4 * ni) + 15) // 16 * 16


def items(a, dtype_name):
    """``[(units, forms, splittable)]`` in the stacked order: fp32 units are tiles of 32 rows, fp64 units are rows."""
    m1, nq, m2, k = a["b1"].size, a["r"].size, a["b2"].size, a["k"]
    rows = [int(r) for r in a["soc_rows"]]
    if dtype_name == "float32":
        out = [(-(-m1 // 32), 0, 1)] + [(2, 1, 0)] * nq + [(2 if r > 32 else 1, 1, 0) for r in rows] + [(-(-m2 // 32), 0, 1)]
    else:
        out = [(m1, 0, 1)] + [(k, 1, 0)] * nq + [(r, 1, 0) for r in rows] + [(m2, 0, 1)]
    return [it for it in out if it[0] > 0]


def partition(its, dtype_name, K, window):
    """Windows as lists of pieces ``(item, first unit, units)``, or None when an item does not fit a window."""
    f64 = dtype_name == "float64"

    def room(units, forms, pieces):
        """The most units a further piece of a run can bring into a window that holds this much."""
        if not f64:
            return (window - bytes32(units, forms)) // TILE_BYTES32
        words = window // 8 - forms * K - 5 * (pieces + 1)          # (the window is a multiple of 16: rounding up never decides)
        return words // (K + 1) - units if words >= 0 else -1

    def size(units, forms, pieces):
        return bytes64(units, forms, pieces, K) if f64 else bytes32(units, forms)

    windows, cur, held = [], [], [0, 0]
    for index, (units, forms, splittable) in enumerate(its):
        if not splittable:
            if size(held[0] + units, held[1] + forms, len(cur) + 1) > window:
                if cur:
                    windows.append(cur)
                    cur, held = [], [0, 0]
                if size(units, forms, 1) > window:
                    return None
            cur.append((index, 0, units))
            held = [held[0] + units, held[1] + forms]
            continue
        done = 0
        while done < units:
            n = min(units - done, room(held[0], held[1], len(cur)))
            if n <= 0:
                if not cur:
                    return None
                windows.append(cur)
                cur, held = [], [0, 0]
                continue
            cur.append((index, done, n))
            held[0] += n
            done += n
    if cur:
        windows.append(cur)
    return windows


def window_bytes_of(window, its, dtype_name, K):
    units = sum(n for _, _, n in window)
    forms = sum(its[i][1] for i, _, _ in window)
    return bytes64(units, forms, len(window), K) if dtype_name == "float64" else bytes32(units, forms)


def smallest_window(a, dtype_name):
    """fp32: two tiles and a form.  fp64: what the set's largest item takes alone (a row of a run, a whole quadratic or cone)."""
    if dtype_name == "float32":
        return MIN_WINDOW32
    K = sweep.lane64_K(a["k"])
    return max(bytes64(1 if split else units, forms, 1, K) for units, forms, split in items(a, dtype_name))


def forced_windows(a, dtype_name):
    """The smallest legal window, three tiles' worth (fp64: three times 32 rows), and 0 = the default."""
    small = smallest_window(a, dtype_name)
    if dtype_name == "float32":
        three = 3 * TILE_BYTES32 + FORM_BYTES32
    else:
        three = max(small, bytes64(96, 1, 3, sweep.lane64_K(a["k"])))
    assert small % 16 == 0 and three % 16 == 0 and small <= three <= DEFAULT_WINDOW
    return (small, three, 0)


def stream_served_by_formula(a, dtype_name, window=0):
    """The envelope: k <= 64; fp32 cones of at most 64 rows; every item within a window (the total within 1 GiB is not
    approached here)."""
    if a["k"] > 64 or (dtype_name == "float32" and max((int(r) for r in a["soc_rows"]), default=0) > 64):
        return False
    its = items(a, dtype_name)
    return bool(its) and partition(its, dtype_name, sweep.lane64_K(a["k"]), window or DEFAULT_WINDOW) is not None


# ------------------------------------------------------------------------------------------------------------------
# sets beyond the resident envelope
# ------------------------------------------------------------------------------------------------------------------

CORRIDOR_K, CORRIDOR_BATCHES = 12, (1, 31, 129, 257)


@functools.lru_cache(maxsize=None)
def corridor_set():
    """Corridor-shaped and small: 700 faces, 40 quadratics, 3 equalities in 12 columns (fp32: 22 + 80 + 1 tiles)."""
    return sweep.random_set(CORRIDOR_K, 700, 40, (), 3, seed=901)


@functools.lru_cache(maxsize=None)
def corridor_case(B=257):
    if B != 257:
        return corridor_case().head(B)
    return sweep.SweepCase("corridor_k12", corridor_set(), sweep.random_rows(CORRIDOR_K, 257, seed=902))


@functools.lru_cache(maxsize=None)
def c5_shape_case():
    """The shape of config 5 (the corridor set): 1 050 faces, 72 quadratics at k = 45, 15 equalities; 129 rows."""
    return sweep.SweepCase("c5_shape", sweep.random_set(45, 1050, 72, (), 15, seed=903), sweep.random_rows(45, 129, seed=904))


@functools.lru_cache(maxsize=None)
def cones_case():
    """30 cones of 33 rows (two tiles each, one valid row in the second) behind 40 linear rows: the two-tile items fall on
    window ends at every window size."""
    return sweep.SweepCase("cones30x33", sweep.random_set(12, 40, 0, (33,) * 30, 1, seed=905), sweep.random_rows(12, 65, seed=906))


@functools.lru_cache(maxsize=None)
def past_limit_case(dtype_name):
    """One row past the largest linear-only image (k = 8) the resident kernel of the precision serves."""
    return sweep.limit_case(sweep.limit_rows(dtype_name) + 1)


def c3_case(name="c3"):
    return cost_cases.case(name)


# name -> (builder, the precisions it runs at)
BEYOND = {
    "past_limit32": (functools.partial(past_limit_case, "float32"), ("float32",)),
    "past_limit64": (functools.partial(past_limit_case, "float64"), ("float64",)),
    "c3": (c3_case, ("float64",)),
    "c3_inside": (functools.partial(c3_case, "c3_inside"), ("float64",)),
    "corridor_k12": (corridor_case, DTYPES),
    "c5_shape": (c5_shape_case, DTYPES),
    "cones30x33": (cones_case, ("float32",)),
}
BEYOND_PARAMS = [(n, d) for n, (_, dtypes) in BEYOND.items() for d in dtypes]


def beyond_case(name):
    return BEYOND[name][0]()


# ------------------------------------------------------------------------------------------------------------------
# a set with an LMI whose rows are beyond the resident fp32 image: 700 linear rows (k = 10) and a 20 x 20 LMI
# ------------------------------------------------------------------------------------------------------------------

LMI_K, LMI_R, LMI_ROWS, LMI_B = 10, 20, 700, 67


@functools.lru_cache(maxsize=None)
def lmi_case():
    """A ``cost_lmi_cases.Case`` (what ``cost_lmi_cases.check`` reads) of a hand-made set; the batch is that module's: rows
    inside, outside, near the LMI's boundary, one NaN row and the degenerate row."""
    c = object.__new__(L.Case)
    c.name, c.B, c.k, c.r, c.cs = "lin700_lmi20", LMI_B, LMI_K, LMI_R, None
    rng = np.random.default_rng(907)
    arrays = sweep.make_set(LMI_K, rng.standard_normal((LMI_ROWS, LMI_K)) / np.sqrt(LMI_K), rng.uniform(0.5, 1.5, size=LMI_ROWS))
    arrays["F"] = np.ascontiguousarray(np.stack(L.generators(LMI_K, LMI_R, 908), axis=0))
    alone = dict(arrays)
    for key in ("A1", "P", "q", "M", "c", "A2", "b1", "r", "s", "d", "soc_rows", "b2"):
        alone[key] = arrays[key][:0]
    c.arrays, c.rows_arrays, c.alone_arrays = arrays, dict(arrays, F=np.zeros((0, 0, 0))), alone
    c.kinds = L._kinds(c.B)
    F = arrays["F"]
    y = np.zeros((c.B, c.k))
    steps = [s * m for m in (1e-5, 1e-9) for s in (0.5, -0.5, 1.0, -1.0, 2.0, -2.0)]
    for b, kind in enumerate(c.kinds):
        u = rng.uniform(-1.0, 1.0, size=c.k)
        if kind == "interior":
            y[b] = 0.02 * u
        elif kind == "outside":
            t0 = L._exit(F, u)
            if t0 is None:
                u = -u
                t0 = L._exit(F, u)
            y[b] = rng.uniform(2.0, 4.0) * (1.0 if t0 is None else t0) * u
        elif kind == "mid":
            y[b] = 0.7 * u
        elif kind == "degenerate":
            y[b, 0] = 1.0
        elif kind == "near":
            at = L._on_ray(F, u, steps[b % len(steps)])
            y[b] = u if at is None else at
        else:
            y[b] = u
            y[b, c.k // 2] = np.nan
    c.y = y
    c.y.setflags(write=False)
    c.ref = L.reference(arrays, y)
    c.finite = ~np.isnan(c.ref["cost"])
    c.degenerate = np.array([kd == "degenerate" for kd in c.kinds])
    c.kept = c.finite & ~c.degenerate & (c.ref["lmi"]["gap"] >= 1e-2)
    c.fnorm = np.array([np.linalg.norm(Fa, 2) for Fa in F[:-1]])
    return c


# ------------------------------------------------------------------------------------------------------------------
# sets both routes serve (the bit-equality test): name -> builder of a case with .arrays and .y
# ------------------------------------------------------------------------------------------------------------------

class _Rows:
    """arrays and rows without a reference (the bit-equality test compares two kernels)."""

    def __init__(self, name, arrays, y):
        self.name, self.arrays, self.y, self.pad = name, arrays, np.ascontiguousarray(y, dtype=np.float64), 0


def _inf():
    y, a = sweep.inf_case()
    return _Rows("inf", a, y)


def shared_cases():
    out = {n: functools.partial(cost_cases.case, n) for n in cost_cases.NAMES}
    out.update({f"tile_{n}": functools.partial(sweep.tile_case, n) for n in sweep.TILE_SETS})
    out.update({f"coverage_{n}": functools.partial(sweep.coverage_case, n) for n in sweep.COVERAGE})
    out.update({f"exact_{n}": fn for n, fn in sweep.EXACT.items()})
    out.update({f"nan_c{c}_r{r}": functools.partial(sweep.nan_case, c, r) for c in sweep.NAN_COLS for r in sweep.NAN_ROWS})
    out["inf"] = _inf
    return out


SHARED = shared_cases()
# what the resident kernels refuse of these (the rest must be served by both routes)
SHARED_REFUSED = {("c3", "float64"), ("c3_inside", "float64"), ("tile_cone65", "float32")}
