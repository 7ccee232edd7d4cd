#!/usr/bin/env python
"""Time method='Bar' (rayen_amd/csrc/rayen_bar.hip) forward and backward with HIP events, next to the reference
formula in eager torch ops on the same GPU, and price the forward against the HBM roofline.

    python scripts/bar_bench.py [--reps 50] [--sets example_00:500,box10:262144,...]

Bytes per forward = B (nv + nr + k) s (q read once, y written once); the backward reads q, grad_y and the row
statistic and writes grad_q: B (2 (nv + nr) + k + 1) s.  The roofline uses 6.3 TB/s, the achievable HBM rate.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rayen_amd import ops, workloads  # noqa: E402
from rayen_amd.constraint_module import ConstraintModule  # noqa: E402

HBM = 6.3e12


def _lin(A, b, k, y0=None):
    raw = workloads._empty(k)
    raw["A1"], raw["b1"] = A, b
    if y0 is not None:
        raw["y0"] = y0
    return raw


def make_set(name):
    if name == "triangle":         # a triangle cut from the cube (the shape of the reference's example 0), k = 3
        A = np.r_[np.eye(3), -np.eye(3)]
        b = np.r_[np.ones(3), np.zeros(3)][:, None]
        raw = _lin(A, b, 3, np.full((3, 1), 0.25))
        raw["A2"], raw["b2"] = np.ones((1, 3)), np.ones((1, 1))
        return raw
    if name == "box10":
        return _lin(np.r_[np.eye(10), -np.eye(10)], np.ones((20, 1)), 10)
    if name == "simplex64":
        return _lin(np.r_[-np.eye(64), np.ones((1, 64))], np.r_[np.zeros(64), [1.0]][:, None], 64, np.full((64, 1), 1 / 128))
    if name == "poly5":
        rng = np.random.default_rng(5)
        D = rng.normal(size=(60, 5))
        return _lin(D / np.linalg.norm(D, axis=1, keepdims=True), np.ones((60, 1)), 5)
    raise ValueError(name)


def time_call(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sets", default="triangle:500,box10:262144,simplex64:262144,poly5:262144,box10:4096")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for item in args.sets.split(","):
        name, B = item.split(":")
        B = int(B)
        layer = ConstraintModule(workloads.build_constraints(make_set(name)), method="Bar", create_map=False).to(dev)
        nv, nr, k = layer.num_vertices, layer.num_rays, layer.k
        m = nv + nr
        bp, pack_id = layer.bar_pack(dev)
        q = torch.randn(B, m, device=dev)
        gy = torch.randn(B, k, device=dev)
        _, rowstat = ops.bar_forward_raw(q, bp)
        fwd = time_call(lambda: ops.bar_forward_raw(q, bp, want_rowstat=False), args.reps)
        bwd = time_call(lambda: ops.bar_backward_raw(q, rowstat, gy, bp), args.reps)
        q3 = q.unsqueeze(2)
        module = time_call(lambda: layer(q3), args.reps)
        with torch.no_grad():
            eager = time_call(lambda: layer._bar_reference(q3), args.reps)
        fbytes = B * (m + k) * 4
        bbytes = B * (2 * m + k + 1) * 4
        print(json.dumps({"set": name, "B": B, "nv": nv, "nr": nr, "k": k, "fwd_ms": fwd * 1e3, "bwd_ms": bwd * 1e3,
                          "module_fwd_ms": module * 1e3, "eager_formula_ms": eager * 1e3,
                          "fwd_TBps": fbytes / fwd / 1e12, "fwd_frac_hbm": fbytes / HBM / fwd,
                          "bwd_TBps": bbytes / bwd / 1e12, "fwd_roofline_ms": fbytes / HBM * 1e3}), flush=True)


if __name__ == "__main__":
    main()
