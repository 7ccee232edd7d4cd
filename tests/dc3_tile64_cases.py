"""Cases, calls and bars for the fp64 DC3 tile kernels (rayen_amd/csrc/rayen_dc3_tile64.hip), built from the reference and
the seeded generators of tests/dc3_reference.py.

Bar.  The project's own fp64 bar: ``dc3_cases.row_err`` against the fp64 host reference at most 1e-11 (``FLOOR[torch.float64]``
of tests/test_gpu_dc3_sweep.py), ``y`` and ``grad_q`` separately; ``steps`` equal to the host's.  Why it fits: the kernels do
exact fp64 arithmetic in another summation order than the host.  The fp64 reference and the same reference with the rows and
the quadratics stacked in reverse order differ by a few 1e-16 in both (tests/test_dc3_tile64_host.py prints the gap per call
and holds it at 1e-13): the bar leaves orders of headroom to summation order and none to a wrong term.

Every row is compared, also in the backward.  That is sound only where no residual at a visited step lies within
``KINK_REL * max(1, max |res|)`` of zero (the backward is discontinuous where a residual changes sign): a condition on the
inputs, which ``sound()`` states and the host test shows for every call the GPU file makes.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import dc3_reference as ref
import dc3_tile_cases as tc

BAR = 1e-11                  # FLOOR[torch.float64] of tests/test_gpu_dc3_sweep.py
REORDER_BAR = 1e-13          # the host reference against itself with another stacking order
KINK_REL = 1e-9
F64 = torch.float64

# what the fp64 lane kernel refuses (n > 32, or an fp64 image over LDS): the ground these kernels are for
BEYOND_CASES = [ref.CASE["np64_n33_nearly_unconstrained"], ref.CASE["np64_n64_five_equalities"], ref.CASE["np64_n64_c3_shape"],
                ref.LDS_CASE["lds_fp32_only"], ref.LDS_CASE["lds_at_the_limit"]] + list(tc.TILE_CASES)
# what it serves: padding of every kind (n = 17: one row into the second 16-row block) and the cross-checks
SMALL_CASES = [ref.CASE["np4_n1_one_inequality"], ref.CASE["np4_n4_quadratics_only"], ref.CASE["np8_n5_ragged_everything"],
               ref.CASE["np32_n17_one_quadratic"], ref.CASE["np32_n32_full"], ref.EQUALITIES_ONLY]
CASES = BEYOND_CASES + SMALL_CASES
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES) == 15

# (B, max_steps, t*) with forward and backward; forward only at B = 257 (t* None: eps = 0, a partial second launch)
BACKWARD_CALLS = [(33, 10, 7), (65, 10, 7), (33, 40, 33)]
FORWARD_CALLS = [(257, 10, 7), (257, 100, 33), (257, 33, None)]

# stop positions around the 32-step launches
POSITION_CASES = ["np8_n5_ragged_everything", "np64_n64_five_equalities"]
POSITIONS = [(32, 32), (33, 33), (33, 32), (100, 1), (100, 33), (100, 64)]
POSITION_BATCH = 33

MATES_CASES = ["tile_n33_forty_quadratics", "np8_n5_ragged_everything"]
MATES_BATCHES = (1, 15, 16, 17, 33, 65)
MATES_STEPS = 10

Call = namedtuple("Call", "arrays q gy lr momentum eps max_steps steps v y64 gq64 nearest")


def never_stops(case):
    """A set without inequalities never meets the stop rule (dc3_reference.forward_ref): it runs to the limit."""
    return case.m + case.nq == 0


def expected_steps(case, max_steps, t_star):
    return max_steps if t_star is None or never_stops(case) else t_star


def nearest_residual(res):
    """min |res| / max(1, max |res|) over every residual at every visited step (inf for a set without inequalities)."""
    res = np.asarray(res, dtype=np.float64)
    if res.size == 0:
        return float("inf")
    return float(np.min(np.abs(res)) / max(1.0, float(np.max(np.abs(res)))))


@functools.lru_cache(maxsize=None)
def call_for(name, B, max_steps, t_star, seed=0, backward=True):
    """One call of case ``name`` with its fp64 host results: eps placed so that the host stops at ``t_star`` (None: eps = 0)."""
    case = CASE[name]
    arrays = ref.make_pack(case)
    q, gy = ref.make_inputs(case, B, seed)
    eps = 0.0
    if t_star is not None and not never_stops(case):
        eps = ref.eps_for(ref.forward_ref(arrays, q, case.lr, ref.MOMENTUM, 0.0, t_star).v, t_star)
    f64 = ref.forward_ref(arrays, q, case.lr, ref.MOMENTUM, eps, max_steps, F64)
    gq = ref.backward_ref(arrays, q, gy, case.lr, ref.MOMENTUM, f64.steps, F64) if backward else np.zeros((B, case.n))
    return Call(arrays, q, gy, case.lr, ref.MOMENTUM, eps, max_steps, f64.steps, f64.v, f64.y, gq, nearest_residual(f64.res))


def forward_call_for(name, B, max_steps, t_star, seed=0):
    return call_for(name, B, max_steps, t_star, seed, False)


def sound(call, backward=True):
    """The conditions a call must meet on the host before a kernel is judged by it; returns what fails (empty: sound)."""
    said = []
    if not (np.isfinite(call.y64).all() and np.isfinite(call.v).all()):
        said.append("not finite")
    if call.eps > 0.0 and not ref.stop_margin(call.v, call.eps, call.steps, call.max_steps):
        said.append("the stop is decided within 0.5 % of eps")
    if backward:
        if not np.isfinite(call.gq64).all():
            said.append("gradient not finite")
        if not call.nearest > KINK_REL:
            said.append(f"a residual within {call.nearest:.1e} (relative) of zero at a visited step")
    return said


def reversed_pack(arrays):
    """The same set with its rows and its quadratics stacked in reverse order: another summation order for the host."""
    out = dict(arrays)
    out["A1e"] = arrays["A1e"][::-1].copy()
    out["b1e"] = arrays["b1e"][::-1].copy()
    out["Pe"] = arrays["Pe"][::-1].copy()
    out["qe"] = arrays["qe"][::-1].copy()
    out["re"] = arrays["re"][::-1].copy()
    return out


def reorder_gap(call):
    """(y, grad_q): ``row_err`` between the fp64 reference of ``call`` and the same on ``reversed_pack``."""
    other = reversed_pack(call.arrays)
    f = ref.forward_ref(other, call.q, call.lr, call.momentum, call.eps, call.max_steps, F64)
    if f.steps != call.steps:
        return float("inf"), float("inf")
    g = ref.backward_ref(other, call.q, call.gy, call.lr, call.momentum, f.steps, F64)
    return float(ref.row_err(f.y, call.y64).max()), float(ref.row_err(g, call.gq64).max())


# ------------------------------------------------------------------------------------------------------------------
# the image layout, restated (Dc3TileLayout64 of rayen_dc3_tile_image.h; its kp is the kp here, kg is not kept there)
# ------------------------------------------------------------------------------------------------------------------

def dims(n, m, nq, no):
    """The offsets (in doubles) and counts of ``rayen::Dc3TileLayout64::dims``."""
    nx, kg = (n + 15) // 16, (n + 3) // 4
    kp, Mb, Cb = (kg + 1) // 2, (m + 15) // 16, (no + 15) // 16
    sizes = [("A", Mb * kp * 128), ("AT", Mb * nx * 256), ("b", Mb * 16), ("P", nq * nx * kp * 128),
             ("PT", nq * nx * kp * 128), ("q", nq * nx * 16), ("r", (nq + 1) // 2 * 2), ("C", Cb * kp * 128),
             ("CT", Cb * nx * 256), ("c0", Cb * 16)]
    d, at = dict(nx=nx, kg=kg, kp=kp, Mb=Mb, Cb=Cb), 0
    for key, size in sizes:
        d["off_" + key] = at
        at += size
    d["total"] = at + 2
    return d


def shape_served(n, m, nq, no):
    return 1 <= n <= 64 and m >= 0 and nq >= 0 and no >= 0 and dims(n, m, nq, no)["total"] * 8 <= 1 << 30


def _at(M, r, c):
    return M[r, c] if r < M.shape[0] and c < M.shape[1] else 0.0


def _rows(M, blocks, kp):
    out = np.zeros(blocks * kp * 128)
    for b in range(blocks):
        for gp in range(kp):
            for lane in range(64):
                for e in range(2):
                    out[((b * kp + gp) * 64 + lane) * 2 + e] = _at(M, 16 * b + (lane & 15), 8 * gp + 4 * e + (lane >> 4))
    return out


def _columns(M, blocks, nx):
    out = np.zeros(blocks * nx * 256)
    for b in range(blocks):
        for ob in range(nx):
            for gp in range(2):
                for lane in range(64):
                    for e in range(2):
                        out[(((b * nx + ob) * 2 + gp) * 64 + lane) * 2 + e] = _at(M, 16 * b + 8 * gp + 4 * e + (lane >> 4),
                                                                                   16 * ob + (lane & 15))
    return out


def image(arrays):
    """The fp64 tile image of a pack as the header's comment states it, element by element."""
    n, k = int(arrays["n"]), int(arrays["k"])
    A, P, C = arrays["A1e"].reshape(-1, n), arrays["Pe"].reshape(-1, n, n), arrays["C"].reshape(-1, n)
    m, nq, no = A.shape[0], P.shape[0], k - n
    d = dims(n, m, nq, no)
    h = np.zeros(d["total"])

    def put(key, values):
        h[d["off_" + key]:d["off_" + key] + len(values)] = values

    put("A", _rows(A, d["Mb"], d["kp"]))
    put("AT", _columns(A, d["Mb"], d["nx"]))
    put("b", arrays["b1e"].reshape(-1))
    for c in range(nq):
        size = d["nx"] * d["kp"] * 128
        h[d["off_P"] + c * size:d["off_P"] + (c + 1) * size] = _rows(P[c], d["nx"], d["kp"])
        h[d["off_PT"] + c * size:d["off_PT"] + (c + 1) * size] = _rows(P[c].T, d["nx"], d["kp"])
        h[d["off_q"] + c * d["nx"] * 16:d["off_q"] + c * d["nx"] * 16 + n] = arrays["qe"].reshape(-1, n)[c]
    put("r", arrays["re"].reshape(-1))
    put("C", _rows(C, d["Cb"], d["kp"]))
    put("CT", _columns(C, d["Cb"], d["nx"]))
    put("c0", arrays["c0"].reshape(-1))
    return h
