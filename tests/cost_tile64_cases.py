"""Cases of the fp64 tile soft cost (rayen_amd/csrc/rayen_cost_tile64.hip): a Python restatement of the block image, its slot
function and the window partition of rayen_amd/csrc/rayen_cost_tile64_layout.h (tests/test_cost_tile64_host.py holds the two
against each other; tests/test_gpu_soft_cost_tile64.py runs the cases), the forced window sizes, and the sets on the row-block
boundaries.

Sets and rows come from ``cost_sweep_cases`` (seeded; the fp64 reference of a case is computed once).  The yardstick of every
GPU test is ``helpers.cost_check(c, 'float64', ...)`` at the bars of tests/cost_reference.py, which hold for any summation
order: no tolerance is introduced here."""
import functools

import numpy as np

import cost_sweep_cases as sweep

ROWS = 16                                   # kCostTile64Rows: rows of a block, samples of a column block
LDS_BUDGET = 160 * 1024
DEFAULT_WINDOW = LDS_BUDGET // 2            # kCostTile64Window
MAX_IMAGE = 1 << 30
TABLE_BYTES = 32                            # per window, in front of the windows


# ------------------------------------------------------------------------------------------------------------------
# the layout, restated
# ------------------------------------------------------------------------------------------------------------------

def width(k):
    """K of the kernel instance for k columns; 0 outside 1 .. 64."""
    if k < 1 or k > 64:
        return 0
    return 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64


def form_width(K):
    return max(K, 16)


def slot(m, c):
    """Word of (row m, column c) inside a block's 16 K words."""
    return (m & 1) | ((c & 1) << 1) | ((((m >> 1) ^ (c >> 1)) & 7) << 2) | ((c >> 1) << 5)


def blocks(rows):
    return -(-rows // ROWS)


def bytes_of(nb, nf, K):
    return (8 * (nb * (16 * K + 16 + 1 + 4) + nf * form_width(K)) + 15) // 16 * 16


def items(a):
    """``[(blocks, forms, splittable)]`` in the stacked order."""
    m1, nq, m2, k = a["b1"].size, a["r"].size, a["b2"].size, a["k"]
    out = [(blocks(m1), 0, 1)] + [(blocks(k), 1, 0)] * nq + [(blocks(int(r)), 1, 0) for r in a["soc_rows"]] + [(blocks(m2), 0, 1)]
    return [it for it in out if it[0] > 0]


def partition(its, K, window):
    """Windows as lists of pieces ``(item, first block, blocks)``, or None when an item does not fit a window (closed forms
    where the header counts block by block)."""
    per_block, KF = 16 * K + 21, form_width(K)

    def room(nb, nf):
        """The most blocks a run can add to a window that holds this much (the window is a multiple of 16: rounding up never
        decides)."""
        return (window // 8 - nf * KF) // per_block - nb

    windows, cur, held = [], [], [0, 0]
    for index, (nb, forms, splittable) in enumerate(its):
        if not splittable:
            if bytes_of(held[0] + nb, held[1] + forms, K) > window:
                if cur:
                    windows.append(cur)
                    cur, held = [], [0, 0]
                if bytes_of(nb, forms, K) > window:
                    return None
            cur.append((index, 0, nb))
            held = [held[0] + nb, held[1] + forms]
            continue
        done = 0
        while done < nb:
            n = min(nb - done, room(held[0], held[1]))
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


def window_bytes_of(window, its, K):
    return bytes_of(sum(n for _, _, n in window), sum(its[i][1] for i, _, _ in window), K)


def smallest_window(a):
    """What the set's largest item takes alone: a block of a run, a whole quadratic or cone."""
    K = width(a["k"])
    return max(bytes_of(1 if split else nb, forms, K) for nb, forms, split in items(a))


def forced_windows(a):
    """The smallest legal window, three blocks' worth, and 0 = the default."""
    small = smallest_window(a)
    three = max(small, bytes_of(3, 1, width(a["k"])))
    assert small % 16 == 0 and three % 16 == 0 and small <= three <= DEFAULT_WINDOW
    return (small, three, 0)


def served_by_formula(a, window=0):
    """The envelope of ``cost_tile64_served``: 1 <= k <= 64, every item within a window, table and windows within 1 GiB."""
    K = width(a["k"])
    its = items(a)
    if K == 0 or not its:
        return False
    cut = partition(its, K, window or DEFAULT_WINDOW)
    return cut is not None and TABLE_BYTES * len(cut) + sum(window_bytes_of(w, its, K) for w in cut) <= MAX_IMAGE


def parity_windows(a):
    """``(window, nw)`` with an odd and with an even number of windows, both > 1: from a workgroup's second pass on, the
    buffer of window 0 alternates when nw is odd and stays when it is even."""
    K, its, found = width(a["k"]), items(a), {}
    window = smallest_window(a)
    while window <= DEFAULT_WINDOW and len(found) < 2:
        nw = len(partition(its, K, window))
        if nw > 1:
            found.setdefault(nw % 2, (window, nw))
        window += bytes_of(1, 0, K) // 16 * 16
    assert set(found) == {0, 1}, found
    return [found[1], found[0]]


# ------------------------------------------------------------------------------------------------------------------
# the lane map of v_mfma_f64_16x16x4_f64, emulated: D [16][16] += A [16][4] B [4][16]
#   A: lane l holds A[l & 15][l >> 4];  B: lane l holds B[l >> 4][l & 15];  C/D: register i of lane l holds D[4 i + (l >> 4)][l & 15]
# ------------------------------------------------------------------------------------------------------------------

def mfma(a_lanes, b_lanes, acc_lanes):
    """One instruction on per-lane operands: ``a_lanes``, ``b_lanes`` [64], ``acc_lanes`` [64][4]; returns the new [64][4]."""
    lanes = np.arange(64)
    A = np.zeros((16, 4))
    Bm = np.zeros((4, 16))
    A[lanes & 15, lanes >> 4] = a_lanes
    Bm[lanes >> 4, lanes & 15] = b_lanes
    D = A @ Bm
    out = np.array(acc_lanes, dtype=np.float64, copy=True)
    for i in range(4):
        out[:, i] += D[4 * i + (lanes >> 4), lanes & 15]
    return out


# ------------------------------------------------------------------------------------------------------------------
# sets on the row-block boundaries (k = 12, 33 rows): runs of 15 .. 33 linear and equality rows, cones of 1 .. 65 rows
# ------------------------------------------------------------------------------------------------------------------

BOUNDARY_K, BOUNDARY_B = 12, 33
RUNS = (15, 16, 17, 31, 32, 33)
CONES = (1, 16, 17, 33, 64, 65)          # one block keeps its products in registers; beyond, they are computed again
BOUNDARY = {f"lin{m}": (m, 1, (3,), 2) for m in RUNS}
BOUNDARY.update({f"eq{m}": (2, 1, (3,), m) for m in RUNS})
BOUNDARY.update({f"cone{r}": (3, 1, (r, 2), 2) for r in CONES})


@functools.lru_cache(maxsize=None)
def boundary_case(name):
    m1, nq, cone_rows, m2 = BOUNDARY[name]
    seed = 1100 + sorted(BOUNDARY).index(name)
    return sweep.SweepCase(f"block_{name}", sweep.random_set(BOUNDARY_K, m1, nq, cone_rows, m2, seed=seed),
                           sweep.random_rows(BOUNDARY_K, BOUNDARY_B, seed=seed + 500))


# a NaN in every lane group (column % 4) and in both column blocks of the first wave, the next wave and the last group
NAN_COLS, NAN_ROWS = (0, 5, 34, 35), (0, 15, 16, 31, 32, 64)


@functools.lru_cache(maxsize=None)
def nan_case(col, row):
    base = sweep.width_case(sweep.NAN_K)
    y = base.y.copy()
    y[row, col] = np.nan
    return sweep.SweepCase(f"nan_c{col}_r{row}", base.arrays, y, kind="nan")


@functools.lru_cache(maxsize=None)
def k8_case():
    """k = 8: linear rows beyond one default window (80 blocks of 1 KiB and their row data), a quadratic, a cone, equalities."""
    return sweep.SweepCase("k8_windows", sweep.random_set(8, 1300, 2, (20,), 5, seed=1201), sweep.random_rows(8, 67, seed=1202))
