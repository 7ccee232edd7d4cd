"""fp64 reference, condition scales and input generators for the Bar kernels (rayen_amd/csrc/rayen_bar.hip).

Plain torch in fp64 on whatever device the arguments live on; nothing here imports ``rayen_amd``.

    y = G [softmax(q[:, :nv]); |q[:, nv:nv+nr]|] + yp                    G: [k, m], m = nv + nr

The error metric divides by what the arithmetic actually adds up (sums of absolute values), not by the result: a peaked
softmax makes the true gradient ``lambda (g - <lambda, g>)`` a cancellation, and an error relative to the result then
measures the conditioning of the input instead of the kernel.  No row is left out and nothing but fp64's ``tiny`` guards
a zero scale.

The sweep's cases and its seeded input generators live here too, so that the host tests (tests/test_bar_reference_host.py)
judge the very inputs the GPU sweep (tests/test_gpu_bar_sweep.py) runs.
"""
import math
from collections import namedtuple

import numpy as np
import torch

TINY = torch.finfo(torch.float64).tiny
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def _f64(t):
    return t.to(torch.float64)


def softmax64(q):
    """Row softmax in fp64 from its definition.  (Not ``torch.softmax``: on the ROCm build this suite runs on, its fp64
    device kernel for rows wider than 1 024 is good to about 5e-10 only -- measured against the host, nv = 1 271 and
    5 111 -- which is seven digits short of what an fp64 kernel is held to here.)"""
    q = _f64(q)
    e = torch.exp(q - torch.max(q, dim=1, keepdim=True).values.detach())
    return e / e.sum(dim=1, keepdim=True)


def weights64(nv, nr, q):
    """``[softmax(q[:, :nv]), |q[:, nv:nv+nr]|]`` in fp64, shape [B, nv + nr]."""
    q = _f64(q)
    parts = []
    if nv:
        parts.append(softmax64(q[:, :nv]))
    if nr:
        parts.append(torch.abs(q[:, nv:nv + nr]))
    return torch.cat(parts, dim=1)


def forward64(G, yp, nv, nr, q):
    return weights64(nv, nr, q) @ _f64(G).t() + _f64(yp).reshape(1, -1)


def backward64(G, nv, nr, q, gy):
    """Closed form of d<gy, y>/dq on the first nv + nr columns: ``lambda (g - <lambda, g>)`` on the vertex columns,
    ``sign(q) g`` on the ray columns (``sign(0) = 0``), ``g = gy G``."""
    q = _f64(q)
    g = _f64(gy) @ _f64(G)
    parts = []
    if nv:
        lam = softmax64(q[:, :nv])
        gv = g[:, :nv]
        parts.append(lam * (gv - (lam * gv).sum(dim=1, keepdim=True)))
    if nr:
        parts.append(torch.sign(q[:, nv:nv + nr]) * g[:, nv:nv + nr])
    return torch.cat(parts, dim=1)


def forward_scale(G, yp, nv, nr, q):
    """``S_i = sum_j |G_ij| w_j + |yp_i|``, shape [B, k]."""
    return weights64(nv, nr, q) @ _f64(G).abs().t() + _f64(yp).abs().reshape(1, -1)


def backward_scale(G, nv, nr, q, gy):
    """``T_j = lambda_j (a_j + sum_l lambda_l a_l)`` on vertex columns, ``a_j`` on ray columns,
    ``a_j = sum_i |G_ij| |gy_i|``; shape [B, nv + nr]."""
    a = _f64(gy).abs() @ _f64(G).abs()
    parts = []
    if nv:
        lam = softmax64(q[:, :nv])
        av = a[:, :nv]
        parts.append(lam * (av + (lam * av).sum(dim=1, keepdim=True)))
    if nr:
        parts.append(a[:, nv:nv + nr])
    return torch.cat(parts, dim=1)


def scaled_err(got, ref, scale):
    """Per row ``max_j |got - ref|_j / max_j scale_j`` (a NaN or an infinity in ``got`` gives a NaN or inf row)."""
    num = torch.max(torch.abs(_f64(got) - _f64(ref)), dim=1).values
    return num / torch.clamp(torch.max(_f64(scale), dim=1).values, min=TINY)


def lse64(nv, q):
    q = _f64(q)[:, :nv]
    top = torch.max(q, dim=1, keepdim=True).values
    return top[:, 0] + torch.log(torch.exp(q - top).sum(dim=1))


# ------------------------------------------------------------------------------------------------------------------
# the sweep's cases
# ------------------------------------------------------------------------------------------------------------------

Case = namedtuple("Case", "name k nv nr")

THREADS = 512                       # the kernels' workgroup size (rayen_bar.hip: kThreads)
LDS_BUDGET = 160 * 1024


def pad_k(k):
    return 4 if k <= 4 else 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64


def pieces(m):
    return (m + 3) // 4


def lanes(m):
    """L: the lanes that share a row (rayen_bar.hip: group_log2)."""
    L = 1
    while L < pieces(m) and L < 16:
        L *= 2
    return L


def rows_per_iter(m):
    return THREADS // lanes(m)


def lds_bytes(m, K, elem):
    return (((m + 3) & ~3) + 1) * K * elem


def tolerance_factor(case):
    """C of the sweep's bar ``C u``: the longest FMA chain of a lane (four terms per piece), a K-term dot product, and
    a constant for the shuffle adds, exp, the normalisation and lse."""
    m = case.nv + case.nr
    return 4 * math.ceil(pieces(m) / lanes(m)) + pad_k(case.k) + 48


# name: L<lanes>_<what it is there for>.  Every K in {4, 8, 16, 32, 64} at its lower and upper k, every L, at least twice.
CASES = [
    Case("L1_k1_single_vertex", 1, 1, 0),              # nv = 1 (weights == 1, gradient == 0), nr = 0, m % 4 = 1
    Case("L1_k3_rays_only", 3, 0, 3),                  # nv = 0, m % 4 = 3
    Case("L1_k4_mixed_piece_one_ray", 4, 3, 1),        # nv % 4 = 3 and nr = 1 in ONE piece
    Case("L2_k5_mixed_piece", 5, 5, 2),                # nv % 4 = 1 with rays, m % 4 = 3
    Case("L2_k8_vertices_only", 8, 6, 0),              # nr = 0, m % 4 = 2
    Case("L4_k9_one_vertex_ten_rays", 9, 1, 10),       # nv = 1 with rays, 3 pieces on 4 lanes, m % 4 = 3
    Case("L4_k16_mixed_piece", 16, 10, 6),             # nv % 4 = 2 with rays, m % 4 = 0
    Case("L8_k17_six_pieces", 17, 18, 3),              # 6 pieces on 8 lanes, nv % 4 = 2, m % 4 = 1
    Case("L8_k32_rays_only", 32, 0, 32),               # nv = 0, 8 pieces on 8 lanes
    Case("L16_k33_ten_pieces", 33, 37, 0),             # 10 pieces on 16 lanes, nr = 0, m % 4 = 1
    Case("L16_k64_simplex_like", 64, 65, 64),          # K = 64 at its upper edge, nv % 4 = 1 with rays
    Case("L16_k8_thousand_generators", 8, 1023, 6),    # >= 1 024 generators, 258 pieces on 16 lanes, nv % 4 = 3
    Case("L16_k16_sixteen_pieces", 16, 40, 24),        # pieces == L, m % 4 = 0
    Case("L16_k32_one_ray", 32, 130, 1),               # nr = 1 behind a ragged vertex piece, m % 4 = 3
    Case("L16_k4_wide", 4, 200, 57),                   # K = 4 with many pieces, m % 4 = 1
]
CASE = {c.name: c for c in CASES}


def _seed(case, *extra):
    return [case.k, case.nv, case.nr, *extra]


def make_pack(case):
    """(G [k, m], yp [k]) as fp64 numpy arrays whose values fp32 holds exactly (so both images of the pack are exact).
    Columns differ in size (0.5 .. 2) and no coefficient is near zero, so a dropped, swapped or misfiled generator
    moves the result; three quarters of a row's coefficients share its sign, so ``<lambda, g>`` does not average out over
    a thousand vertices."""
    rng = np.random.default_rng(_seed(case, 1))
    m = case.nv + case.nr
    size = 0.5 + 1.5 * ((np.arange(m) * 7) % 11) / 10.0
    sign = rng.choice([-1.0, 1.0], size=(case.k, 1)) * np.where(rng.random(size=(case.k, m)) < 0.75, 1.0, -1.0)
    G = sign * rng.uniform(0.5, 1.0, size=(case.k, m)) * size[None, :]
    yp = rng.choice([-1.0, 1.0], size=case.k) * rng.uniform(0.5, 1.5, size=case.k)
    return (np.ascontiguousarray(G.astype(np.float32).astype(np.float64)),
            np.ascontiguousarray(yp.astype(np.float32).astype(np.float64)))


def make_inputs(case, B, variant="plain", amplitude=5.0, width=None, seed=0):
    """(q [B, width >= m], gy [B, k]) as fp64 numpy arrays of fp32-representable values: logits uniform in
    +-amplitude, gy standard normal.  ``variant='edges'`` scatters exact zeros over the ray columns and -inf over the
    vertex columns (never a whole row).  Columns beyond m hold NaN."""
    rng = np.random.default_rng(_seed(case, 2, B, int(amplitude), seed))
    m = case.nv + case.nr
    width = m if width is None else width
    q = np.full((B, width), np.nan)
    q[:, :m] = rng.uniform(-amplitude, amplitude, size=(B, m))
    gy = rng.standard_normal(size=(B, case.k))
    if variant == "edges":
        hit = rng.random(size=(B, m)) < 0.25
        rows = np.arange(B)
        if case.nv > 1:
            hit[rows, rows % case.nv] = False              # one finite vertex logit per row at least
        else:
            hit[:, :case.nv] = False
        q[:, :case.nv][hit[:, :case.nv]] = -np.inf
        q[:, case.nv:m][hit[:, case.nv:]] = 0.0
    elif variant != "plain":
        raise ValueError(variant)
    return q.astype(np.float32).astype(np.float64), gy.astype(np.float32).astype(np.float64)


def sweep_batches(case, cus=None):
    """The sweep's batch sizes: 1, one short of and one past a workgroup's rows; with ``cus`` also one that makes every
    workgroup of a full grid take a second trip of its row loop."""
    rpi = rows_per_iter(case.nv + case.nr)
    out = [1, rpi - 1, rpi + 1]
    if cus is not None:
        out.append(cus * 4 * rpi + rpi + 3)
    return out
