"""Three seeded cases beyond the wave kernel's envelope (more than 576 cone rows, more than 32 cones) for the tile kernel
(rayen_amd/csrc/rayen_proj_tile.hip).  The fp64 reference of tests/proj_reference.py takes 25 to 70 s per case on the
host, so its results -- and the fp32 host mirror's -- are fixtures: tests/golden/proj_tile/<name>.npz, written by
tests/golden/proj_tile/make_fixtures.py.  Importing this module registers the cases in ``proj_reference.CASE`` (so
``make_cs``, ``make_inputs``, ``module_for`` serve them); ``compare`` and ``bars`` are ``proj_reference``'s, fed from the
fixtures."""
import functools
import os

import numpy as np

import proj_reference as pr
from rayen_amd import workloads

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proj_tile")

CASES = [
    pr.Case("n8_rows_past_576", lambda: workloads.random_lin_quad_soc(8, 640, 0, 0, seed=11), 0.1),
    pr.Case("n8_mixed_past_576", lambda: workloads.random_lin_quad_soc(8, 590, 2, 1, seed=14), 0.15),
    pr.Case("n6_forty_cones", lambda: workloads.corridor_like(k=10, n_eq=4, m=20, n_quad=40, rank=2, seed=12), 0.3),
]
NAMES = [c.name for c in CASES]
# (n, cone rows m, cones) of each case's program
SHAPE = {"n8_rows_past_576": (8, 640, 0), "n8_mixed_past_576": (8, 619, 3), "n6_forty_cones": (6, 180, 40)}
for _case in CASES:
    pr.CASE.setdefault(_case.name, _case)


def fixture_path(name, golden=GOLDEN):
    return os.path.join(golden, name + ".npz")


@functools.lru_cache(maxsize=None)
def fixture(name, golden=GOLDEN):
    with np.load(fixture_path(name, golden)) as f:
        return {k: f[k] for k in f.files}


# a fixture's keys of the host mirror's run, by precision (the fp64 run is recorded where a kernel serves the case in fp64)
MIRROR_KEYS = {"float32": "mirror", "float64": "mirror64"}


@functools.lru_cache(maxsize=None)
def reference(name, golden=GOLDEN, B=pr.BATCH):
    """``proj_reference.Reference`` of a case from its fixture of ``B`` rows (the inputs are checked against
    ``make_inputs``)."""
    f = fixture(name, golden)
    q, gy = pr.make_inputs(name, B)
    assert np.array_equal(f["q"], q) and np.array_equal(f["gy"], gy), "fixture inputs are not make_inputs'"
    return pr.Reference(q, gy, f["z"], f["grad_q"], f["margin"], f["margin"] < pr.KINK_MARGIN, f["interior"].astype(bool))


def mirror_run(name, dtype_name="float32", golden=GOLDEN):
    """The host mirror's run at ``dtype_name`` recorded in the fixture."""
    f, key = fixture(name, golden), MIRROR_KEYS[dtype_name]
    return pr.Run(f[key + "_z"], f[key + "_grad_q"], f[key + "_iters"])


def save_fixture(path, ref, runs, **extra):
    """Write a fixture: the reference, the mirror's runs ``{dtype_name: pr.Run}`` and what else a case table records."""
    arrays = dict(q=ref.q, gy=ref.gy, z=ref.z, grad_q=ref.grad_q, margin=ref.margin, interior=ref.interior, **extra)
    for dtype_name, run in runs.items():
        key = MIRROR_KEYS[dtype_name]
        arrays.update({key + "_z": run.z, key + "_grad_q": run.grad_q, key + "_iters": run.iters})
    np.savez_compressed(path, **arrays)


def install(name, golden=GOLDEN, B=pr.BATCH, dtype_names=("float32",)):
    """Put the fixture's results where ``pr.reference`` / ``pr.mirror_run`` would compute them (their caches): after this
    ``pr.compare`` and ``pr.bars`` serve the case at ``dtype_names`` like any other."""
    _seed_cache(pr.reference, (name,), reference(name, golden, B))
    for dtype_name in dtype_names:
        _seed_cache(pr.mirror_run, (name, dtype_name), mirror_run(name, dtype_name, golden))


_SEEDED = {}


def _seed_cache(cached, key, value, module=pr):
    """``functools.lru_cache`` offers no insertion: wrap the cached function of ``module`` once with a table looked up
    first (``.inner`` of the wrapper is the function it wraps)."""
    table = _SEEDED.get((module.__name__, cached.__name__))
    if table is None:
        table = _SEEDED[(module.__name__, cached.__name__)] = {}
        inner = getattr(module, cached.__name__)

        def outer(*args, _inner=inner, _table=table, **kwargs):
            return _table[args] if not kwargs and args in _table else _inner(*args, **kwargs)
        outer.__name__ = cached.__name__
        outer.inner = inner
        setattr(module, cached.__name__, outer)
    table[key] = value


def bars(name):
    install(name)
    return pr.bars(name, "float32")


def compare(name, z, grad_q, iters, rows=None):
    install(name)
    return pr.compare(name, "float32", z, grad_q, iters, rows=rows)
