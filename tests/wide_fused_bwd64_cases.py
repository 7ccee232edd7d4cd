"""The sets and inputs of the fp64 fused wide backward's tests (tests/test_wide_fused_bwd64_host.py,
tests/test_gpu_wide_fused_bwd64.py), a Python restatement of rayen_amd/csrc/rayen_wide_fused_bwd64_layout.h, and a host
restatement of the backward formula in ``np.longdouble``.

    case         what it exercises
    mixI, mixE   (wide_fused_bwd_cases, inputs and upstream gradients cast to double) every segment type is the active one;
                 16-row blocks of 16 / 16 / 6 rows (a 38-row QUAD_FAC), a 3-row segment, a 41-row cone; mixE: NA_E != I with
                 k % 16 = 14
    n65          (wide_fused64_cases) the smallest wide fp64 n; kp = 72: two chunks and one group; segments of 17 / 65 / 17
                 rows, each one row past a block
    plan_a       (wide_fused64_cases, relaid) a cone's aux rows at rows 15 | 16: blocks 0 | 1
    plan_c       (wide_fused64_cases, relaid) QUAD_FAC segments of 17 / 1 / 15 / 16 rows
    s32_last     the largest n of the edge family (20 linear rows and a cone of 5, whatever n) whose BACKWARD plan picks 32
                 samples, found from the restated plan (``s32_last_n``)
    s16_first    the next n: 16 samples
    k1024        (wide_fused_cases) the envelope's last n, a dense QUAD_SYM: 16 samples
    k1025        (wide_fused_cases) one past it: the refusal

Inputs.  mixI / mixE / k1024: those of wide_fused_bwd_cases, as doubles.  The others -- the forward's inputs of
wide_fused64_cases leave the cone of n65, the 17-row segment of plan_c and one cone of plan_a active on no row -- get
``own_inputs``: 300 rows uniform in [-1, 1] (torch generator, seed ``SEED[name]``) times ``ROW_SCALE[row % 5]``, rows 96-127
times 1e-3 (tiles in which nobody is clipped).  Which segment a row activates does not depend on its length, so every
non-linear segment of these sets is active on some rows (tests/test_wide_fused_bwd64_host.py counts them).
Upstream gradients: uniform in [-1, 1], seed 177 (those of wide_fused_bwd_cases, drawn as doubles for the sets of this file)."""
import functools

import numpy as np
import torch

import wide_fused64_cases as C64
import wide_fused_bwd_cases as CB
import wide_fused_cases as F
from rayen_amd import _lib

MIXED = ("mixI", "mixE")
SMALL = ("n65", "plan_a", "plan_c")
EDGES = ("s32_last", "s16_first")
CASES = (*MIXED, *SMALL, *EDGES, "k1024")
BITS = (*MIXED, *EDGES)                       # the cases of the bit-equality tests
B = 300
SEED = {"n65": 641, "plan_a": 642, "plan_c": 643, "s32_last": 644, "s16_first": 645}
ROW_SCALE = (0.02, 0.05, 0.1, 0.2, 0.4)

# ---------------------------------------------------------------- the layout header, restated
MAX_N, LDS = 1024, 160 * 1024 - 256
pad8, widest_t, perm_offset, workspace = CB.pad8, CB.widest_t, CB.perm_offset, CB.workspace
PLAN_KEYS = ("kp", "ks", "ke", "gs", "rp", "ts", "np", "samples", "region_words", "lds_bytes", "served")


def scratch(S):
    return 10 * S


def plan(n, k, out_identity, widest, samples=0):
    """The header's ``wide_fused_bwd64_plan`` in Python.  ``samples``: 0 (32 where the LDS fits, else 16), or 16 / 32 forced."""
    kp, ke = pad8(n), 0 if out_identity else pad8(k)
    ks, gs = kp + 2, 0 if out_identity else ke + 2
    rp = pad8(widest) if widest > 0 else 0
    ts = rp + 2 if widest > 0 else 0
    envelope = 1 <= n <= MAX_N and k >= 1 and 0 <= widest <= 1 << 24 and k <= 1 << 24 and samples in (0, 16, 32)
    for S in ((16,) if samples == 16 else (32,) if samples == 32 else (32, 16)):
        region = max(S * gs, S * ks + S * ts)
        lds = 8 * (region + scratch(S))
        served = int(envelope and lds <= LDS)
        if served:
            break
    return dict(kp=kp, ks=ks, ke=ke, gs=gs, rp=rp, ts=ts, np=(n + 15) // 16 * 16, samples=S,
                region_words=region if served else 0, lds_bytes=lds, served=served)


def plan_of(c, samples=0):
    """The restated plan of a pack (``PackedConstants``)."""
    return plan(c.n, c.k, int(c.out_identity), widest_t(c.segments), samples)


# ---------------------------------------------------------------- the sets
@functools.lru_cache(maxsize=None)
def s32_last_n():
    """The largest n of wide_fused64_cases' edge family whose backward plan picks 32 samples: searched with the restated plan
    (the family's segment table -- 20 linear rows and a cone of 5 -- does not depend on n:
    tests/test_wide_fused_bwd64_host.py checks it on the sets built)."""
    picks = [n for n in range(65, MAX_N + 1) if plan(n, n, 1, 5)["samples"] == 32]
    assert picks and picks == list(range(65, picks[-1] + 1)) and picks[-1] < MAX_N
    return picks[-1]


@functools.lru_cache(maxsize=None)
def cs(name):
    from rayen_amd import workloads
    if name in MIXED:
        return CB.cs(name)
    if name in SMALL:
        return C64.cs(name)
    if name in EDGES:
        return workloads.build_constraints(C64._edge_raw(s32_last_n() + (name == "s16_first")))
    return F.cs(name)                         # k1024, k1025


@functools.lru_cache(maxsize=None)
def packed(name):
    """The packer's own layout of a case's set (what the module runs)."""
    from rayen_amd.constraint_module import ConstraintModule
    return ConstraintModule(cs(name), create_map=False).packed_constants()


@functools.lru_cache(maxsize=None)
def consts(name):
    """The pack of a case on which the records are made: the relaid layout of plan_a / plan_c, else the packer's."""
    return C64.consts(name) if name in ("plan_a", "plan_c") else packed(name)


def own_inputs(n, seed, batch=B):
    gen = torch.Generator().manual_seed(seed)
    x = torch.empty(B, n, dtype=torch.float64).uniform_(-1, 1, generator=gen)
    x *= torch.tensor(ROW_SCALE, dtype=torch.float64)[torch.arange(B) % len(ROW_SCALE)][:, None]
    x[96:128] *= 1e-3
    return x[:batch].clone()


def inputs(name, batch=B):
    """``[batch, n]`` fp64."""
    if name in SEED:
        return own_inputs(cs(name).n, SEED[name], batch)
    return CB.inputs(name, batch)[:, :, 0].double()


def grads(name, batch=B):
    """``[batch, k]`` fp64 upstream gradients, uniform in [-1, 1]."""
    if name in MIXED or name == "k1024":
        return CB.grads(name, batch).double()
    gen = torch.Generator().manual_seed(177)
    return torch.empty(B, cs(name).k, dtype=torch.float64).uniform_(-1, 1, generator=gen)[:batch].clone()


# ---------------------------------------------------------------- what the inputs exercise, in fp64 on the host
@functools.lru_cache(maxsize=None)
def coverage(name):
    """Of a case's inputs on its pack: clipped rows; per segment index the rows on which it is active; distinct active
    non-linear segments per tile of 16 rows in batch order; tiles of 16 in which nobody is clipped."""
    c = consts(name)
    v = inputs(name).numpy()
    kappa, seg = CB.active64(c, v)
    clipped = kappa > 1
    rows = {i: np.flatnonzero(clipped & (seg == i)) for i in range(len(c.segments))}
    nonlin = np.array([s >= 0 and c.segments[s].type != _lib.SEG_LIN for s in seg.tolist()])
    per_tile, unclipped_tiles = [], 0
    for t in range(0, len(v), 16):
        m = clipped[t:t + 16] & nonlin[t:t + 16]
        per_tile.append(len(set(seg[t:t + 16][m].tolist())))
        unclipped_tiles += int(not clipped[t:t + 16].any())
    return dict(clipped=int(clipped.sum()), rows=rows, per_tile=per_tile, unclipped_tiles=unclipped_tiles)


# ---------------------------------------------------------------- the backward formula, restated in np.longdouble
def reference(c, v, kappa, active, G):
    """grad_v ``[B, n]`` (np.longdouble) of the RAYEN step from the packed constants ``c`` and the recorded ``kappa [B]``,
    ``active [B, 2]``: s = 1 / max(1, kappa), u = NA_E' g, coef = -s^2 (u . v) where kappa > 1, and the active constraint's
    combination of rows of W (rayen_amd/csrc/rayen_wide_fused_bwd.hip states the closers)."""
    L = np.longdouble
    W, v, G, kappa = c.W.astype(L), np.asarray(v).astype(L), np.asarray(G).astype(L), np.asarray(kappa).astype(L)
    U = G if c.out_identity else G @ c.NA_E.astype(L)
    out = np.empty_like(v)
    for b in range(v.shape[0]):
        kap, u, x = kappa[b], U[b], v[b]
        s = L(1) / max(L(1), kap)
        g = s * u
        seg = int(active[b, 0])
        if kap > 1 and 0 <= seg < len(c.segments):
            coef = -s * s * (u @ x)
            sg = c.segments[seg]
            rows = W[sg.row0:sg.row0 + sg.nrows]
            if sg.type == _lib.SEG_LIN:
                row = int(active[b, 1])
                if sg.row0 <= row < sg.row0 + sg.nrows:
                    g = g + coef * W[row]
            elif sg.type in (_lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC):
                T = rows @ x
                cvec = x[:sg.nrows] if sg.type == _lib.SEG_QUAD_SYM else T
                rad = np.sqrt(max(T @ cvec, L(0)))
                so = coef / rad if rad > 0 else L(0)
                g = g + coef * W[sg.aux_row] + so * (cvec @ rows)
            elif sg.type == _lib.SEG_SOC:
                T = rows @ x
                cr, br = W[sg.aux_row] @ x, W[sg.aux_row + 1] @ x
                bp = 2 * br - 2 * cr * L(sg.f0)
                den = 2 * L(sg.f1) * kap + bp
                q = coef / den if den != 0 else L(0)
                g = g + q * (2 * L(sg.f0) * kap + 2 * cr) * W[sg.aux_row] - 2 * q * kap * W[sg.aux_row + 1] - 2 * q * (T @ rows)
        out[b] = g
    return out
