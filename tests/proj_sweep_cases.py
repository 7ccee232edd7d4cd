"""Seeded cases at the boundaries of the two Euclidean-projection kernels (rayen_amd/csrc/rayen_proj.hip: wave per sample,
fp32 and fp64; rayen_amd/csrc/rayen_proj_tile.hip: 32 samples per workgroup, fp32), and restatements of their launch rules.

Every case is ``workloads.random_lin_quad_soc(k, m, n_quad, n_soc, r_M, seed)``: its program has
``m + n_quad (k + 2) + n_soc (r_M + 1)`` rows, so a boundary is hit exactly.  The batch is the leading 97 rows of
``proj_reference.make_inputs``: 24 wave groups plus one row, three tiles plus one row.  The fp64 reference
(``proj_reference.reference``: ``conic.solve`` at 1e-11, KKT Jacobian) and the host mirror's fp32 and fp64 runs are fixtures,
tests/golden/proj_sweep/<name>.npz, written by tests/golden/proj_sweep/make_fixtures.py and read through the helper of
tests/proj_tile_cases.py.  Importing this module registers the cases in ``proj_reference.CASE``; ``compare`` and ``bars`` are
``proj_reference``'s.

What each case is there for (R: rows of v a lane of the wave kernel holds, 1 / 3 / 9 at m <= 64 / <= 192 / above; tile: blocks
per wave of the layout -> the instance (NB, NX) that runs it):

  name              args (k, m, nq, ns, r_M)  program (n, m, cones)  R  tile           what it hits
  m64               (8, 34, 2, 1, 9)          (8, 64, 3)             1  1 -> (2, 1)    R = 1 full, m % 4 == 0 (mpad = m + 1), last t in lane 63
  m65               (8, 35, 2, 1, 9)          (8, 65, 3)             3  1 -> (2, 1)    R = 3, one row in register 1: the last cone's t at i = 64,
                                                                                       that cone across lanes 55..63 -> lane 0
  m192              (8, 100, 2, 1, 71)        (8, 192, 3)            3  3 -> (6, 1)    R = 3 full; a 72-row cone (a lane holds two of its rows)
  m193              (8, 101, 2, 1, 71)        (8, 193, 3)            9  3 -> (6, 1)    R = 9, one row in register 3: t at i = 192
  m576              (8, 476, 2, 1, 79)        (8, 576, 3)            9  5 -> (6, 1)    kMaxRows; fp64 R = 9 without a PSD block (64 KiB of LDS)
  soc32             (6, 4, 0, 32, 2)          (6, 100, 32)           3  2 -> (2, 1)    kMaxSoc
  soc33             (6, 4, 0, 33, 2)          (6, 103, 33)           -  2 -> (2, 1)    the wave kernel refuses; 'auto' and 'tile' serve it
  nolin_five_cones  (8, 0, 3, 2, 8)           (8, 48, 5)             1  1 -> (2, 1)    m_lin = 0 with several cones
  t2_n8_full        (8, 224, 1, 1, 9)         (8, 244, 2)            9  2 -> (2, 1)    256 re-laid rows: the (2, 1) instance full
  t3_n8             (8, 225, 1, 1, 9)         (8, 245, 2)            9  3 -> (6, 1)    the first shape past them
  t7_n8             (8, 780, 2, 1, 8)         (8, 809, 3)            -  7 -> (12, 1)   the first layout of the parked-p instance at n <= 32
  t7_n33            (33, 700, 1, 1, 33)       (33, 769, 2)           -  7 -> (10, 2)   the first layout of the parked-p instance at n > 32
                                                                                       (mostly interior: 14 of the 97 rows lie outside the set)
  t12_n8_full       (8, 1472, 1, 1, 25)       (8, 1508, 2)           -  12 -> (12, 1)  every block of the largest layout in use
  t10_n33_full      (33, 1180, 1, 1, 33)      (33, 1249, 2)          -  10 -> (10, 2)  the same at n > 32
                                                                                       (mostly interior: 12 of the 97 rows lie outside the set)
  t7_n33_deep, t10_n33_full_deep: the two programs above at amp 0.03 (59 and 69 rows outside, 5 and 12 kink rows: over the
  cap), kept for the FORWARD comparison alone; the backward of the (10, 2) instance is judged on the gentler batches.

The other instances have their cases in tests/proj_reference.py (n33_padding_lanes: tile (2, 2); n64_c3_shape: tile (6, 2),
wave fp32 R = 9) and tests/proj_lmi_reference.py (the PSD instantiations at R = 1 and R = 9); DESIGN.md lists all of them.
R = 3 with a PSD block (a block of 11 .. 18 rows) had no case: ``r12_k5`` below, 33 seeded rows, is registered in
``proj_lmi_reference.CASE`` and served by that module's reference, mirror, ``bars`` and ``compare`` (all under a second each
on the host, so it has no fixture).
"""
# Measured: row_gap against the fp64 reference, forward / backward on the non-kink rows, and iterations max / mean, on the 97
# seeded rows (r12_k5: 33).  Host: the mirror (what the bars are KINK_FACTOR times of; tests/golden/proj_sweep/make_fixtures.py
# prints these).  Device: MI355X, tests/test_gpu_proj_sweep.py (it prints them); "=" where wave and tile agree to the digits shown.
#                     kink  host mirror fp32            host mirror fp64             wave fp32                   wave fp64                    tile fp32
#   case              rows  fwd     bwd     iters       fwd     bwd     iters        fwd     bwd     iters       fwd     bwd     iters        fwd     bwd     iters
#   m64               0     5.4e-5  1.4e-4  224 / 110   5.4e-8  1.7e-7  454 / 241    5.3e-5  1.4e-4  225 / 110   5.4e-8  1.7e-7  454 / 241    5.3e-5  1.5e-4  225 / 110
#   m65               0     1.2e-5  1.6e-5  131 / 51    1.5e-8  2.4e-8  223 / 91     1.2e-5  1.7e-5  130 / 51    1.5e-8  2.4e-8  223 / 91     1.2e-5  1.7e-5  130 / 51
#   m192              0     1.1e-5  5.4e-5  310 / 142   1.1e-8  4.9e-8  564 / 277    1.0e-5  5.4e-5  310 / 142   1.1e-8  4.9e-8  564 / 277    1.0e-5  5.4e-5  310 / 142
#   m193              0     1.3e-5  5.9e-5  308 / 147   1.3e-8  6.3e-8  569 / 283    1.3e-5  5.8e-5  294 / 147   1.3e-8  6.3e-8  569 / 283    1.3e-5  5.8e-5  294 / 147
#   m576              1     2.3e-5  1.4e-4  698 / 422   3.1e-8  2.2e-7  1400 / 894   2.3e-5  1.9e-4  697 / 422   3.1e-8  2.2e-7  1400 / 894   2.3e-5  1.3e-4  697 / 422
#   soc32             0     7.4e-6  4.0e-5  186 / 99    1.9e-8  6.1e-8  365 / 181    7.3e-6  1.9e-5  186 / 99    1.9e-8  6.1e-8  365 / 181    7.2e-6  4.0e-5  186 / 99
#   soc33             0     9.3e-5  1.3e-4  436 / 230   -                            refused                     refused                      9.6e-5  1.2e-4  436 / 230
#   nolin_five_cones  0     3.8e-5  1.4e-4  149 / 72    3.9e-8  1.1e-7  309 / 154    3.8e-5  1.4e-4  148 / 72    3.9e-8  1.1e-7  309 / 154    3.8e-5  1.4e-4  148 / 72
#   t2_n8_full        0     7.8e-6  1.0e-4  311 / 176   2.0e-8  1.3e-7  640 / 355    8.1e-6  1.0e-4  311 / 176   2.0e-8  1.3e-7  640 / 355    8.0e-6  1.0e-4  311 / 176
#   t3_n8             0     2.4e-5  6.3e-5  365 / 190   3.7e-8  7.1e-8  793 / 379    2.4e-5  6.3e-5  365 / 191   3.7e-8  7.1e-8  793 / 379    2.4e-5  6.2e-5  365 / 191
#   t7_n8             0     3.2e-6  2.2e-4  401 / 191   -                            refused                     refused                      6.1e-6  2.2e-4  401 / 192
#   t7_n33            0     4.6e-5  1.0e-4  302 / 30    -                            refused                     refused                      4.6e-5  9.4e-5  304 / 30
#   t12_n8_full       1     7.1e-6  8.1e-6  780 / 404   -                            refused                     refused                      7.0e-6  7.8e-6  781 / 404
#   t10_n33_full      0     4.2e-5  4.5e-4  368 / 30    -                            refused                     refused                      4.2e-5  4.8e-4  368 / 31
#   t7_n33_deep       5     1.1e-4  (fwd)   487 / 192   -                            refused                     refused                      1.2e-4  (fwd)   487 / 192
#   t10_n33_full_deep 12    1.7e-4  (fwd)   720 / 334   -                            refused                     refused                      1.7e-4  (fwd)   720 / 334
#   r12_k5            0     1.3e-5  8.4e-5  126 / 39    1.4e-8  1.3e-7  225 / 66     8.9e-6  7.4e-5  127 / 39    1.4e-8  1.3e-7  225 / 66     refused (a PSD block)
# The amplitudes are what keeps the kink rows within kink_cap(97) = 2 and the fp64 mirror under MAX_ITERS: with 700 and more
# dense orthant rows many samples end near a vertex (t7_n33 at amp 0.03: 6 kink rows; t10_n33_full: 9; t7_n8 at 0.15: 4 and a
# row at the cap), so t7_n33 and t10_n33_full run at amp 0.012, where 83 and 85 of the 97 rows are inside and 14 and 12 outside;
# their _deep twins at amp 0.03 face the forward's comparisons alone.
import os
from collections import namedtuple

import numpy as np

import proj_lmi_reference as plr
import proj_reference as pr
import proj_tile_cases as ptc
from rayen_amd import workloads

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proj_sweep")
BATCH = 97                           # 24 groups of the wave kernel + 1 row; 3 tiles + 1 row
F32, F64 = "float32", "float64"

Sweep = namedtuple("Sweep", "name args amp seed shape R tile backward", defaults=(True,))


# args: (k, m, n_quad, n_soc, r_M, builder's seed); amp, seed: of make_inputs; shape: (n, m, cones) of the program; R: the
# wave kernel's rows per lane (None: refused); tile: (blocks per wave of the layout, (NB, NX) of the instance)
SWEEP = [
    Sweep("m64", (8, 34, 2, 1, 9, 31), 0.2, 0, (8, 64, 3), 1, (1, (2, 1))),
    Sweep("m65", (8, 35, 2, 1, 9, 32), 0.2, 0, (8, 65, 3), 3, (1, (2, 1))),
    Sweep("m192", (8, 100, 2, 1, 71, 33), 0.2, 0, (8, 192, 3), 3, (3, (6, 1))),
    Sweep("m193", (8, 101, 2, 1, 71, 34), 0.2, 0, (8, 193, 3), 9, (3, (6, 1))),
    Sweep("m576", (8, 476, 2, 1, 79, 35), 0.15, 3, (8, 576, 3), 9, (5, (6, 1))),
    Sweep("soc32", (6, 4, 0, 32, 2, 36), 0.3, 0, (6, 100, 32), 3, (2, (2, 1))),
    Sweep("soc33", (6, 4, 0, 33, 2, 37), 0.3, 0, (6, 103, 33), None, (2, (2, 1))),
    Sweep("nolin_five_cones", (8, 0, 3, 2, 8, 38), 0.3, 0, (8, 48, 5), 1, (1, (2, 1))),
    Sweep("t2_n8_full", (8, 224, 1, 1, 9, 39), 0.1, 1, (8, 244, 2), 9, (2, (2, 1))),
    Sweep("t3_n8", (8, 225, 1, 1, 9, 40), 0.15, 0, (8, 245, 2), 9, (3, (6, 1))),
    Sweep("t7_n8", (8, 780, 2, 1, 8, 41), 0.05, 0, (8, 809, 3), None, (7, (12, 1))),
    Sweep("t7_n33", (33, 700, 1, 1, 33, 42), 0.012, 2, (33, 769, 2), None, (7, (10, 2))),
    Sweep("t12_n8_full", (8, 1472, 1, 1, 25, 43), 0.1, 1, (8, 1508, 2), None, (12, (12, 1))),
    Sweep("t10_n33_full", (33, 1180, 1, 1, 33, 44), 0.012, 3, (33, 1249, 2), None, (10, (10, 2))),
    # the two programs above at amp 0.03, where 59 and 69 of the 97 rows lie outside the set: 5 and 12 kink rows, over the cap, so
    # these batches are kept for the forward alone and the backward is judged on the gentler ones above
    Sweep("t7_n33_deep", (33, 700, 1, 1, 33, 42), 0.03, 0, (33, 769, 2), None, (7, (10, 2)), False),
    Sweep("t10_n33_full_deep", (33, 1180, 1, 1, 33, 44), 0.03, 0, (33, 1249, 2), None, (10, (10, 2)), False),
]
BY_NAME = {s.name: s for s in SWEEP}
NAMES = [s.name for s in SWEEP]
SHAPE = {s.name: s.shape for s in SWEEP}
WAVE_NAMES = [s.name for s in SWEEP if s.R is not None]
# (case, precision) the wave kernel serves: every wave case in both
WAVE_RUNS = [(name, dtype_name) for name in WAVE_NAMES for dtype_name in (F32, F64)]


def _raw(args):
    k, m, nq, ns, r_M, seed = args
    return lambda: workloads.random_lin_quad_soc(k, m, nq, ns, r_M, seed=seed)


for _sweep in SWEEP:
    pr.CASE.setdefault(_sweep.name, pr.Case(_sweep.name, _raw(_sweep.args), _sweep.amp, _sweep.seed))


# the one case with a PSD block: r = 12, 78 svec rows -> R = 3 (rho: the value build_program chose on the host)
LMI_R3 = "r12_k5"
LMI_R3_SHAPE = (5, 78, 0, 12)        # (n, m, cones, r)
plr.CASE.setdefault(LMI_R3, plr.Case(LMI_R3, lambda: workloads.random_lmi(5, 12, seed=3), 0.8, 33, 3.0))
plr.SHAPE.setdefault(LMI_R3, LMI_R3_SHAPE)


# r32_k4 of tests/proj_lmi_reference.py, the stride test's case with a PSD block: its reference and fp64 mirror (12 s on
# the host) are recorded next to the sweep cases' fixtures
LMI_STRIDE = "r32_k4"


def install_lmi(name=LMI_STRIDE):
    """Put the fixture of an LMI case where ``plr.reference`` / ``plr.mirror_run`` (fp64) would compute them."""
    f = ptc.fixture(name, GOLDEN)
    q, gy = plr.make_inputs(name)
    assert np.array_equal(f["q"], q) and np.array_equal(f["gy"], gy), "fixture inputs are not make_inputs'"
    ref = plr.Reference(q, gy, f["z"], f["grad_q"], f["margin"], f["margin"] < plr.KINK_MARGIN, f["interior"].astype(bool),
                        f["nullity"])
    ptc._seed_cache(plr.reference, (name,), ref, plr)
    ptc._seed_cache(plr.mirror_run, (name, F64), plr.Run(*ptc.mirror_run(name, F64, GOLDEN)), plr)
    return ref


def dtype_names(name):
    """The precisions a fixture records the mirror at: fp64 only where the wave kernel serves the case."""
    return (F32, F64) if BY_NAME[name].R is not None else (F32,)


def fixture_path(name):
    return ptc.fixture_path(name, GOLDEN)


def install(name):
    ptc.install(name, GOLDEN, BATCH, dtype_names(name))


def reference(name):
    return ptc.reference(name, GOLDEN, BATCH)


def mirror_run(name, dtype_name):
    return ptc.mirror_run(name, dtype_name, GOLDEN)


def bars(name, dtype_name):
    install(name)
    return pr.bars(name, dtype_name)


def compare(name, dtype_name, z, grad_q, iters, rows=None):
    """``pr.compare``; the forward's comparisons alone for a case kept for its forward (``backward`` false in SWEEP)."""
    install(name)
    return pr.compare(name, dtype_name, z, grad_q, iters, rows=rows, backward=BY_NAME[name].backward)


# ------------------------------------------------------------------------------------------------------------------
# the launch rules, restated (rayen_proj.hip: run, dims_of, launch_as)
# ------------------------------------------------------------------------------------------------------------------

LDS_BUDGET = 160 * 1024               # kLdsBudget
MAX_GRID_PER_CU, CUS = 8, 256


def R_of(m):
    """Rows of v per lane: the instantiation ``run`` picks."""
    return 1 if m <= 64 else 3 if m <= 192 else 9


def psd_scratch(r):
    return 96 + 3 * pr.round4(r * (r | 1)) if r else 0


def wave_lds_bytes(n, m, psd_dim, elem):
    image = pr.round4(n * (m | 1)) + pr.round4(n * n) + pr.round4(m) + pr.round4(n)
    return (image + pr.WAVES * (128 + pr.round4(m) + psd_scratch(psd_dim))) * elem


WaveGrid = namedtuple("WaveGrid", "lds per_cu grid groups per_workgroup scan_passes")


def wave_grid(n, m, psd_dim, elem, B):
    """What ``launch_as`` launches for a batch of ``B``: bytes of LDS, workgroups per CU the cap assumes, the grid, the
    groups of four rows, the most groups one workgroup owns (> 1: the ``group += gridDim.x`` loop runs) and the passes of
    the leave-early scan (its 256 threads cover 64 groups of a workgroup per pass)."""
    lds = wave_lds_bytes(n, m, psd_dim, elem)
    per_cu = min(max(LDS_BUDGET // (lds + 256), 1), MAX_GRID_PER_CU)
    groups = -(-B // pr.WAVES)
    grid = min(groups, CUS * per_cu)
    per_workgroup = -(-groups // grid)
    return WaveGrid(lds, per_cu, grid, groups, per_workgroup, -(-per_workgroup // 64))


def stride_batch(grid):
    """The smallest batch in which workgroup 0 owns three whole groups and workgroup 1's third group is ragged."""
    return pr.WAVES * (2 * grid + 1) + 1


def tile_instance(nb, n):
    """``instance_blocks`` of rayen_proj_tile.hip: (NB, NX)."""
    nx = -(-n // 32)
    return (2 if nb <= 2 else 6 if nb <= 6 else 12 if nx == 1 else 10), nx


# the smallest batch of n3_box (eight workgroups a CU: grid 2048) whose leave-early scan takes a second pass, ragged
SCAN_BATCH = pr.WAVES * (64 * CUS * MAX_GRID_PER_CU + 1) + 1


def tiled_index(rows, B, seed=5):
    """``[B]`` indices into a seeded batch of ``rows``: whole copies of it, each in its own fixed permutation, then its
    leading rows in order.  Every row of the large batch has a twin in the small one, and every copy is the whole seeded
    batch, so ``compare`` serves it."""
    rng = np.random.default_rng([rows, B, seed])
    copies, tail = divmod(B, rows)
    return np.concatenate([rng.permutation(rows) for _ in range(copies)] + [np.arange(tail)]).astype(np.int64)


def launch_classes(iters, chunk=pr.CHUNK):
    """``(inside, early, late)`` rows of a seeded batch whose forward took ``iters``: rows that take no iteration, the rows
    outside that finish in the earliest launch any of them finishes in (the first, where the case has such rows: the seeded
    cases beyond a few rows need more than ``chunk`` iterations for every row outside), and the rows that go on after it."""
    iters = np.asarray(iters)
    launches = -(-iters // chunk)
    first = launches[iters > 0].min()
    classes = tuple(np.flatnonzero(sel) for sel in (iters == 0, (iters > 0) & (launches == first), launches > first))
    assert all(c.size for c in classes), [c.size for c in classes]
    return classes


def grouped_index(iters, B):
    """``[B]`` indices into a seeded batch whose forward took ``iters``, in a repeating pattern of five groups of four: a
    group of interior rows (finished in the first launch without an iteration), a group of early rows, a group of late
    ones, and two groups in which live rows alternate with finished ones."""
    inside, early, late = launch_classes(iters)
    pattern = "iiii" "eeee" "llll" "lile" "elil"
    pools, at = {"i": inside, "e": early, "l": late}, {"i": 0, "e": 0, "l": 0}
    out = np.empty(B, dtype=np.int64)
    for b in range(B):
        kind = pattern[b % len(pattern)]
        out[b] = pools[kind][at[kind] % pools[kind].size]
        at[kind] += 1
    return out


def scan_second_pass_index(iters, B, grid, chunk=pr.CHUNK):
    """``[B]`` indices into a seeded batch whose forward took ``iters`` in which ONLY the second pass of the leave-early
    scan keeps workgroups 0 and 1 alive after the first launch: the groups their first pass covers (``b + k grid``,
    ``k < 64``) hold interior rows alone (finished in the first launch, forward and backward), and the groups past them
    (``64 grid`` and ``64 grid + 1``, the batch's last rows) hold rows that need more than ``chunk`` iterations.  Everything
    else is ``tiled_index``.  A scan that stopped after one pass, or looked at another group in its second, would let
    those two workgroups leave, and their last rows would never be answered."""
    iters = np.asarray(iters)
    inside, late = np.flatnonzero(iters == 0), np.flatnonzero(iters > chunk)
    assert inside.size and late.size
    index = tiled_index(len(iters), B)
    first_pass = np.array([pr.WAVES * (b + k * grid) + w for b in (0, 1) for k in range(64) for w in range(pr.WAVES)])
    second_pass = np.arange(pr.WAVES * 64 * grid, B)
    assert first_pass.max() < second_pass.min() and 1 <= second_pass.size - pr.WAVES <= pr.WAVES
    index[first_pass] = np.resize(inside, first_pass.size)
    index[second_pass] = np.resize(late[np.argsort(-iters[late], kind="stable")], second_pass.size)
    return index, first_pass, second_pass
