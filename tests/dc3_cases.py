"""Shared loading of the ``golden/dc3/dc3_*.npz`` fixtures (tests/golden/make_golden_dc3.py) for the DC3 test files."""
import glob
import os

import numpy as np
import torch

from helpers import GOLDEN
from rayen_amd import workloads
from rayen_amd.constraint_module import ConstraintModule

NAMES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, "dc3", "dc3_*.npz")))
MODES = ("train", "eval")
BUFFERS = ("A2_DC3", "b2_DC3", "A1_DC3", "b1_DC3", "A2oi", "A2p", "A1_effective", "b1_effective", "all_P_effective",
           "all_q_effective", "all_r_effective")


def load(name):
    z = dict(np.load(os.path.join(GOLDEN, "dc3", name + ".npz")))
    raw = workloads._empty(int(z["raw_y0"].shape[0]))
    for key in ("A1", "b1", "A2", "b2"):
        if "raw_" + key in z:
            raw[key] = z["raw_" + key]
    for key in ("P", "q", "r"):
        raw[key] = list(z["raw_" + key]) if "raw_" + key in z else []
    raw["y0"] = z["raw_y0"]
    lr, momentum, eps, t_train, t_eval = z["args"]
    args = dict(lr=float(lr), momentum=float(momentum), eps_converge=float(eps), max_steps_training=int(t_train),
                max_steps_testing=int(t_eval))
    return raw, args, z


def layer_for(name, dtype=torch.float32, args=None):
    """A fresh ``ConstraintModule(method='DC3')`` of the fixture's set, built at ``dtype`` as the default dtype (the
    reference evaluates its buffers there)."""
    raw, fixture_args, z = load(name)
    previous = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        layer = ConstraintModule(workloads.build_constraints(raw), method="DC3", create_map=False,
                                 args_DC3=dict(fixture_args if args is None else args))
    finally:
        torch.set_default_dtype(previous)
    return layer, z


def row_err(y, ref):
    """Per-row error relative to the row's largest magnitude."""
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.max(np.abs(y - ref), axis=1) / np.maximum(np.max(np.abs(ref), axis=1), 1e-30)
