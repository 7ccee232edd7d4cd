"""The sets and inputs of the fused wide backward's tests (tests/test_wide_fused_bwd_host.py,
tests/test_gpu_wide_fused_bwd.py), a Python restatement of rayen_amd/csrc/rayen_wide_fused_bwd_layout.h, and the fp64
bookkeeping on the host that says which constraint is active where.

Cases: ``k129`` (odd K tail) and ``k1024`` (envelope edge, a dense QUAD_SYM) of tests/wide_fused_cases.py with its inputs, and
two mixed sets in which every segment type gets to be the active one:

    raw   = workloads.random_lin_quad_soc(k, m=40, n_quad=2, n_soc=3, r_M=41, seed), the two dense P multiplied by 0.002,
            plus low-rank quadratics P = w 2 C'C, C uniform in [-1, 1] of rank 3 (w = 0.1) and rank 37 (w = W37),
            q uniform in [-1, 1], r uniform in [-1, -0.1] (numpy default_rng(seed + 1000), in that order)
    mixI  k = 160, seed 97, NA_E = I
    mixE  k = 190, seed 98, 30 equality rows uniform in [-1, 1] (default_rng(seed + 2000)) with b2 = 0: n = 160, NA_E != I,
          k no multiple of 32
    W37 = 0.5 in both (at 0.03 the 38-row QUAD_FAC segment was active on no row of mixI and on one row of mixE)
    x     = wide_fused_cases.inputs(n, 300) with rows 9 onward x 0.4, rows 4-7 x 0.04, rows 96-127 x 1e-3 (a whole tile in
            which nobody is clipped); in every case row 8, zero in the forward's inputs, is 1e-3 x row 10 (interior): the
            oracle's autograd gives NaN at v = 0

Counts of the final recipe (``coverage(name)``: fp64 candidates from the packed constants, ``helpers.kink_mask`` at 1e-4;
tests/test_wide_fused_bwd_host.py holds them to the conditions the GPU tests rely on):

    case    clipped rows   LIN / SYM / FAC / SOC active   of those on segments > 32 rows   distinct active segments per tile   kink rows
    mixI    263 of 300     184 / 11 / 58 / 10             184 / 11 / 27 / 10               4 to 6 (one tile: 0)                1
    mixE    263 of 300     198 /  3 / 46 / 16             198 /  3 / 46 / 16               2 to 5 (one tile: 0)                0"""
import functools

import numpy as np
import torch

import wide_fused_cases as F
from rayen_amd import _lib, workloads

CASES = ("k129", "k1024", "mixI", "mixE")
MIXED = {"mixI": dict(k=160, seed=97, n_eq=0, w37=0.5), "mixE": dict(k=190, seed=98, n_eq=30, w37=0.5)}


@functools.lru_cache(maxsize=None)
def raw(name):
    if name not in MIXED:
        return F.raw(name)
    m = MIXED[name]
    k = m["k"]
    r = workloads.random_lin_quad_soc(k=k, m=40, n_quad=2, n_soc=3, r_M=41, seed=m["seed"])
    r["P"] = [0.002 * P for P in r["P"]]
    rng = np.random.default_rng(m["seed"] + 1000)
    for rank, w in ((3, 0.1), (37, m["w37"])):
        Cm = rng.uniform(-1.0, 1.0, size=(rank, k))
        r["P"].append(w * 2.0 * Cm.T @ Cm)
        r["q"].append(rng.uniform(-1.0, 1.0, size=(k, 1)))
        r["r"].append(rng.uniform(-1.0, -0.1, size=(1, 1)))
    if m["n_eq"]:
        r["A2"] = np.random.default_rng(m["seed"] + 2000).uniform(-1, 1, (m["n_eq"], k))
        r["b2"] = np.zeros((m["n_eq"], 1))
    return r


@functools.lru_cache(maxsize=None)
def cs(name):
    return workloads.build_constraints(raw(name))


def inputs(name, B=300):
    """``[B, n, 1]`` fp32 of a case."""
    n = cs(name).n
    x = F.inputs(n, 300)
    x[8] = 1e-3 * x[10]          # (the forward's zero row: fp64 autograd through the oracle has no gradient at v = 0)
    if name in MIXED:
        x[9:] *= 0.4
        x[4:8] *= 0.04
        x[96:128] *= 1e-3
    return x[:B].clone()


def grads(name, B=300):
    """``[B, k]`` fp32 upstream gradients, uniform in [-1, 1]."""
    gen = torch.Generator().manual_seed(177)
    return torch.empty(300, cs(name).k, dtype=torch.float32).uniform_(-1, 1, generator=gen)[:B].clone()


# ---------------------------------------------------------------- which constraint is active, in fp64 on the host
def candidates64(consts, v):
    """fp64 candidates of every segment: a list of ``[B, nrows]`` (linear rows) or ``[B, 1]`` arrays, by segment index."""
    T = v @ consts.W.T
    out = []
    for s in consts.segments:
        rows = T[:, s.row0:s.row0 + s.nrows]
        if s.type == _lib.SEG_LIN:
            out.append(rows)
        elif s.type == _lib.SEG_QUAD_SYM:
            out.append((T[:, s.aux_row] + np.sqrt(np.maximum(np.sum(rows * v[:, :s.nrows], axis=1), 0.0)))[:, None])
        elif s.type == _lib.SEG_QUAD_FAC:
            out.append((T[:, s.aux_row] + np.sqrt(np.sum(rows * rows, axis=1)))[:, None])
        else:
            assert s.type == _lib.SEG_SOC
            cr, br = T[:, s.aux_row], T[:, s.aux_row + 1]
            cp = np.sum(rows * rows, axis=1) - cr * cr
            bp = 2 * br - 2 * cr * s.f0
            disc = bp * bp - 4 * s.f1 * cp
            root = np.sqrt(np.maximum(disc, 0.0))
            cand = np.maximum((-bp - root) / (2 * s.f1), (-bp + root) / (2 * s.f1))
            out.append(np.where(disc >= 0, cand, 0.0)[:, None])
    return out


def assert_active_names_a_maximiser(consts, v, k64, active):
    """The rule of tests/test_gpu_wide_fused.py::test_kappa_and_active_against_fp64_on_the_same_pack: the constraint a
    kernel's ``active [B, 2]`` names is a maximiser in fp64 within 1e-5 max(1, kappa64) (near-ties may pick another row).
    ``v [B, n]`` fp64, ``k64 [B]`` the fp64 kappa of the same pack."""
    cands = candidates64(consts, v)
    scale = np.maximum(1.0, k64)
    for b in range(v.shape[0]):
        seg, row = int(active[b, 0]), int(active[b, 1])
        if k64[b] <= 0:
            assert seg == -1, (b, seg)
            continue
        assert 0 <= seg < len(cands), (b, seg)
        s = consts.segments[seg]
        if s.type == _lib.SEG_LIN:
            assert s.row0 <= row < s.row0 + s.nrows, (b, seg, row)
            named = cands[seg][b, row - s.row0]
        else:
            assert row == 0
            named = cands[seg][b, 0]
        assert k64[b] - named <= 1e-5 * scale[b], (b, seg, row, k64[b], named)


def active64(consts, v):
    """(kappa [B], active segment [B] (-1: none)) in fp64."""
    cands = candidates64(consts, v)
    best = np.stack([c.max(axis=1) for c in cands], axis=1)
    seg = best.argmax(axis=1)
    kappa = np.maximum(best.max(axis=1), 0.0)
    return kappa, np.where(kappa > 0, seg, -1)


@functools.lru_cache(maxsize=None)
def coverage(name):
    """What the inputs of a case exercise: clipped rows, clipped rows by the active segment's type, by (type, nrows > 32),
    distinct active segments (linear ones counted once each) per tile of 32 rows in batch order, unclipped tiles."""
    from rayen_amd.constraint_module import ConstraintModule
    consts = ConstraintModule(cs(name), create_map=False).packed_constants()
    v = inputs(name)[:, :, 0].double().numpy()
    kappa, seg = active64(consts, v)
    clipped = kappa > 1
    by_type, wide = {}, {}
    for b in np.flatnonzero(clipped):
        s = consts.segments[seg[b]]
        by_type[s.type] = by_type.get(s.type, 0) + 1
        if s.nrows > 32:
            wide[s.type] = wide.get(s.type, 0) + 1
    per_tile, unclipped_tiles = [], 0
    for t in range(0, len(v), 32):
        c = clipped[t:t + 32]
        per_tile.append(len(set(seg[t:t + 32][c].tolist())))
        unclipped_tiles += int(not c.any())
    return dict(clipped=int(clipped.sum()), by_type=by_type, wide=wide, per_tile=per_tile, unclipped_tiles=unclipped_tiles)


# ---------------------------------------------------------------- the layout header, restated
MAX_N, LDS, SCRATCH = 1024, 160 * 1024 - 256, 10 * 32


def pad8(x):
    return (x + 7) // 8 * 8


def widest_t(segments):
    """Rows of the widest QUAD_FAC / SOC segment of a packed set (0: none)."""
    return max([int(s.nrows) for s in segments if s.type in (_lib.SEG_QUAD_FAC, _lib.SEG_SOC)], default=0)


def plan(n, k, out_identity, widest):
    kp, ke = pad8(n), 0 if out_identity else pad8(k)
    ks, gs = kp + 4, 0 if out_identity else ke + 4
    rp = pad8(widest) if widest > 0 else 0
    ts = rp + 4 if widest > 0 else 0
    region = max(32 * gs, 32 * ks + 32 * ts)
    lds = 4 * (region + SCRATCH)
    served = int(1 <= n <= MAX_N and k >= 1 and 0 <= widest <= 1 << 24 and k <= 1 << 24 and lds <= LDS)
    return dict(kp=kp, ks=ks, ke=ke, gs=gs, rp=rp, ts=ts, np=(n + 31) // 32 * 32, region_words=region if served else 0,
                lds_bytes=lds, served=served)


def perm_offset(n_keys):
    return (4 * n_keys + 255) // 256 * 256


def workspace(n_nonlinear, B):
    return 0 if n_nonlinear < 2 or B <= 0 else perm_offset(n_nonlinear + 1) + 4 * B


def slots_bwd(plan, cus):
    """Workgroups of the fused backward resident at once: as many a CU as LDS holds, at most three; ``cus`` =
    ``wide_fused_cases.launch_cus(...)``.  The grid is ``wide_fused_cases.grid(B, slots)``."""
    return cus * min(3, max(1, (160 * 1024) // plan["lds_bytes"]))


def grouping_grid(B, cus):
    """Workgroups of the count and scatter kernels: one per 256 rows, at most one per SIMD (they stride beyond)."""
    return min(-(-B // 256), 4 * cus)
