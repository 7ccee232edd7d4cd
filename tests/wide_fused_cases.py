"""The sets and inputs of the fused wide forward's tests (tests/test_wide_fused_host.py, tests/test_gpu_wide_fused.py), and
a Python restatement of the block plan in rayen_amd/csrc/rayen_wide_fused_layout.h."""
import functools

import numpy as np
import torch

from rayen_amd import _lib, workloads

#   name        what it exercises
#   k129        odd K tail one past the threshold; a linear run one row past a block
#   k130        a single row: three waves own nothing
#   k190_n160   NA_E rows, k not a multiple of 32, y as scratch
#   k800        the set of test_gpu_parity.py::test_large_subspace_dimension
#   k1024       the envelope's last n
CASES = ("k129", "k130", "k190_n160", "k800", "k1024")


@functools.lru_cache(maxsize=None)
def raw(name):
    if name == "k129":
        return workloads.random_lin_quad_soc(k=129, m=33, n_quad=1, n_soc=1, r_M=33, seed=91)
    if name == "k130":
        return workloads.random_lin_quad_soc(k=130, m=1, n_quad=0, n_soc=0, seed=92)
    if name == "k190_n160":
        r = workloads.random_lin_quad_soc(k=190, m=70, n_quad=2, n_soc=2, r_M=40, seed=93)
        r["A2"] = np.random.default_rng(90).uniform(-1, 1, (30, 190))
        r["b2"] = np.zeros((30, 1))
        return r
    if name == "k800":
        return workloads.random_lin_quad_soc(k=800, m=120, n_quad=2, n_soc=1, r_M=50, seed=71)
    if name == "k1024":
        return workloads.random_lin_quad_soc(k=1024, m=200, n_quad=1, n_soc=1, r_M=65, seed=94)
    if name == "k1025":                 # one past the envelope (the refusal tests)
        return workloads.random_lin_quad_soc(k=1025, m=3, n_quad=0, n_soc=0, seed=95)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def cs(name):
    return workloads.build_constraints(raw(name))


def inputs(n, B=300):
    """``[B, n, 1]`` fp32: uniform in [-1, 1]; rows 0-3 scaled by 1e-4 (interior), rows 4-7 by 300, row 8 zero."""
    gen = torch.Generator().manual_seed(12)
    x = torch.empty(300, n, 1, dtype=torch.float32).uniform_(-1, 1, generator=gen)
    x[0:4] *= 1e-4
    x[4:8] *= 300
    x[8] = 0
    return x[:B].clone()


# ---------------------------------------------------------------- the block plan, restated
TILE, WAVES, MAX_N, LDS = 32, 4, 1024, 160 * 1024 - 256


def block_start(nb, w):
    return nb * w // WAVES


def wave_of(nb, b):
    for w in range(WAVES):
        if block_start(nb, w) <= b < block_start(nb, w + 1):
            return w
    return -1


def seg_inputs(segments):
    """(row0, nrows, slots, naux) of every segment of a packed set (``rayen_amd.pack.PackedConstants.segments``)."""
    out = []
    for s in segments:
        naux = 1 if s.type in (_lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC) else 2 if s.type == _lib.SEG_SOC else 0
        out.append((int(s.row0), int(s.nrows), 2 if s.type == _lib.SEG_LIN else 1, naux))
    return out


def plan(n, k, n_rows, out_identity, segs):
    """The header's ``wide_fused_plan`` in Python: (plan dict, list of per-segment dicts)."""
    kp = (n + 7) // 8 * 8
    ks = kp + 4
    rows_w_pad = (n_rows + 31) // 32 * 32
    nb_w = rows_w_pad // 32
    rows_e_pad = 0 if out_identity else (k + 31) // 32 * 32
    words = 0
    seg_plans = []
    for row0, nrows, slots, naux in segs:
        first = row0 // 32 if nrows > 0 else 0
        last = (row0 + nrows - 1) // 32 if nrows > 0 else -1
        wf = wave_of(nb_w, first) if nrows > 0 else 0
        wl = wave_of(nb_w, last) if nrows > 0 else -1
        part_off = words
        words += (wl - wf + 1) * slots * 32
        aux_off = words
        words += naux * 32
        seg_plans.append(dict(first_block=first, last_block=last, wave_first=wf, wave_last=wl, part_off=part_off,
                              aux_off=aux_off))
    tile_bytes = 4 * 32 * ks
    lds = tile_bytes + 4 * words + 4 * 2 * 32
    p = dict(n=n, kp=kp, ks=ks, rows_w_pad=rows_w_pad, nb_w=nb_w, rows_e_pad=rows_e_pad, nb_e=rows_e_pad // 32,
             rows_pad=rows_w_pad + rows_e_pad, scratch_words=words, tile_bytes=tile_bytes, lds_bytes=lds,
             served=int(1 <= n <= MAX_N and k >= 1 and lds <= LDS))
    return p, seg_plans


# ---------------------------------------------------------------- the launcher's grid, restated
def launch_cus(cus, reserved=0):
    """Compute units the persistent grids may fill (``launch_simds() / 4``): all but the reserved ones, at least one."""
    return max(1, cus - reserved)


def slots_fwd(plan, cus):
    """Workgroups resident at once: as many a CU as LDS holds, at most four; ``cus`` = ``launch_cus(...)``."""
    return cus * min(4, max(1, (160 * 1024) // plan["lds_bytes"]))


def grid(B, slots):
    """``persistent_grid(B, 32, slots, 1)`` of rayen_launch_geometry.h: the tiles dealt in equal rounds."""
    n_tiles = -(-B // TILE)
    rounds = -(-n_tiles // slots)
    return -(-n_tiles // rounds)
