"""The cases of the fp64 tile kernel of the Euclidean projection (rayen_amd/csrc/rayen_proj_tile64.hip) that no fp64 kernel
served before it, and so whose fixtures carry no fp64 run of the host mirror: the three cases of tests/proj_tile_cases.py
(257 rows) and the boundary cases of tests/proj_sweep_cases.py beyond the wave kernel's envelope (97 rows).  Their fp64
reference is in the existing fixtures; the fp64 mirror's run (up to 50 s a case on the host) is recorded in
tests/golden/proj_tile64/<name>.npz by tests/golden/proj_tile64/make_fixtures.py.  ``install`` puts both where
``proj_reference.compare`` / ``bars`` look, so every case faces the comparisons every kernel faces, at fp64."""
import functools
import os

import numpy as np

import proj_reference as pr
import proj_sweep_cases as psc
import proj_tile_cases as ptc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proj_tile64")
F64 = "float64"

TILE_NAMES = list(ptc.NAMES)
# sweep cases the wave kernel refuses (no fp64 mirror in tests/golden/proj_sweep); the two _deep batches are the same
# programs again and stay with the fp32 kernel
SWEEP_BEYOND = ["soc33", "t7_n8", "t7_n33", "t12_n8_full", "t10_n33_full"]
# sweep cases whose own fixtures carry the fp64 mirror's run
SWEEP_WAVE = list(psc.WAVE_NAMES)
RECORDED = TILE_NAMES + SWEEP_BEYOND


def rows_of(name):
    return psc.BATCH if name in psc.BY_NAME else pr.BATCH


def fixture_path(name):
    return os.path.join(GOLDEN, name + ".npz")


@functools.lru_cache(maxsize=None)
def mirror_run(name):
    """The fp64 host mirror's run on the seeded batch of ``name``: recorded here, or in the sweep's own fixture."""
    if name in SWEEP_WAVE:
        return psc.mirror_run(name, F64)
    with np.load(fixture_path(name)) as f:
        return pr.Run(f["mirror64_z"], f["mirror64_grad_q"], f["mirror64_iters"])


def install(name):
    if name in psc.BY_NAME:
        psc.install(name)
    elif name in ptc.NAMES:
        ptc.install(name)
    else:
        return                                   # a case of proj_reference.CASES: computed on the host, as always
    if name in RECORDED:
        ptc._seed_cache(pr.mirror_run, (name, F64), mirror_run(name))


def reference(name):
    install(name)
    return pr.reference(name)


def host_mirror(name):
    install(name)
    return pr.mirror_run(name, F64)


def bars(name, capped=True):
    install(name)
    return pr.bars(name, F64, capped)


def compare(name, z, grad_q, iters, rows=None, capped=True):
    install(name)
    backward = psc.BY_NAME[name].backward if name in psc.BY_NAME else True
    return pr.compare(name, F64, z, grad_q, iters, rows=rows, capped=capped, backward=backward)
