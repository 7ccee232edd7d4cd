"""Seeded cases of the soft-cost tests (host and GPU), with their fp64 reference computed once and shared.

Small on purpose: the sizes are the ones at which the kernels take another path -- k below, at and one past the 16-byte
piece and the 32-column half (3, 5, 7, 17, 64), rows one past a tile (33 linear rows, a cone of 33 rows), cones of one and of
two tiles, batches of 1, 31, 64, 65 and 257 rows (a partial group, whole groups, one past, several groups with a partial
last one), a row stride above k, rows all inside, all outside, and one NaN row."""
import functools

import numpy as np

from rayen_amd import workloads
from rayen_amd.soft_cost import set_arrays

import cost_reference


def _trim_first_cone(raw, rows):
    raw["M"][0] = raw["M"][0][:rows]
    raw["s"][0] = raw["s"][0][:rows]
    raw["d"][0] = np.linalg.norm(raw["s"][0]) + np.array([[0.5]])
    return raw


def _raws():
    return {
        "box3": workloads.cube(),
        "lin5_eq2": workloads.corridor_like(k=5, n_eq=2, m=7, n_quad=0, rank=1, seed=11),
        "quad_soc7": _trim_first_cone(workloads.random_lin_quad_soc(k=7, m=0, n_quad=1, n_soc=2, r_M=5, seed=12), 2),
        "k17_m33": workloads.random_lin_quad_soc(k=17, m=33, n_quad=3, n_soc=1, r_M=33, seed=13),
        "c3": workloads.make_raw("c3", seed=0),
    }


# name -> (set, B, kind, row stride - k)
_SPECS = {
    "box3": ("box3", 1, "mixed", 0),
    "lin5_eq2": ("lin5_eq2", 31, "mixed", 0),
    "quad_soc7": ("quad_soc7", 64, "mixed", 0),
    "k17_m33": ("k17_m33", 65, "mixed", 0),
    "c3": ("c3", 257, "mixed", 0),
    "k17_strided": ("k17_m33", 65, "mixed", 3),
    "c3_inside": ("c3", 64, "inside", 0),
    "quad_soc7_outside": ("quad_soc7", 31, "outside", 0),
    "k17_nan": ("k17_m33", 65, "nan", 0),
}
NAMES = tuple(_SPECS)
NAN_ROW = 33


class Case:
    def __init__(self, name, cs, arrays, y, pad, kind):
        self.name, self.cs, self.arrays, self.y, self.pad, self.kind = name, cs, arrays, y, pad, kind
        self.ref = cost_reference.reference(arrays, y)
        self.y.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _set(set_name):
    cs = workloads.build_constraints(_raws()[set_name])
    return cs, set_arrays(cs)


@functools.lru_cache(maxsize=None)
def case(name):
    set_name, B, kind, pad = _SPECS[name]
    cs, arrays = _set(set_name)
    rng = np.random.default_rng(sum(map(ord, name)))
    y0 = np.asarray(cs.y0, dtype=np.float64).reshape(1, cs.k)
    span = 1.0 + float(np.max(np.abs(y0)))
    if kind == "inside":
        y = y0 + 1e-3 * rng.uniform(-1.0, 1.0, size=(B, cs.k))
    elif kind == "outside":
        y = y0 + span * rng.uniform(2.0, 4.0, size=(B, cs.k)) * rng.choice([-1.0, 1.0], size=(B, cs.k))
    else:       # rows from well inside to well outside
        y = y0 + span * rng.uniform(-1.0, 1.0, size=(B, cs.k)) * rng.choice([0.02, 0.3, 1.5], size=(B, 1))
    if kind == "nan":
        y[NAN_ROW, cs.k // 2] = np.nan
    return Case(name, cs, arrays, y, pad, kind)
