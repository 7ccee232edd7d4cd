#!/usr/bin/env python
"""Time the fp64 DC3 tile kernels (rayen_amd/csrc/rayen_dc3_tile64.hip) against what served the same fp64 call before them.
The sibling of scripts/bench_dc3_tile.py (fp32), same method.

    python scripts/bench_dc3_tile64.py [--steps 10] [--parts a,b,c] [--out profiles/bench/dc3_tile64.txt]

(a) the c2-shaped set of scripts/dc3_bench.py, B = 262 144: tile64 against the fp64 lane kernel (rayen_dc3.hip) of the same
    build, through ``ops.dc3_forward_raw`` / ``ops.dc3_backward_raw``.  For the record: ``'auto'`` keeps the lane kernel there.
(b) the c3-shaped set (config 3's cones dropped: n = 64, which the fp64 lane kernel refuses) through ``ConstraintModule``,
    B = 262 144: ``args_DC3['kernel'] = 'auto'`` against the reference's iteration in eager torch ops in fp64
    (``_dc3_reference`` and autograd through it), which is all that served an fp64 call on this set before.
(c) the corridor set (config 5) through ``ConstraintModule``, B = 16 384 and 262 144, likewise.

fp64, ``eps_converge = 0`` pins the step count, inputs and lr as in scripts/dc3_bench.py.  Timing: HIP events around windows
of calls; the two paths alternate in one process, and a path's figure is the mean of its last window once two consecutive
windows of it agree within 2 % (``settled`` says whether they did within the round limit).  A path whose first call takes
longer than ``--slow-ms`` (the eager route at the large batches) is timed one call a window, its first call counting as a
window.  Useful flops per row: forward ``T (4 m n + nq (2 n^2 + 4 n))``; backward ``(T - 1)`` forward steps again plus
``T (6 m n + nq (4 n^2 + 8 n))``; the share is against the 78.6 TFLOP/s fp64 matrix peak of the MI355X (bench.py's
``PEAK_FP64_TFLOPS``).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rayen_amd import dc3, ops, workloads  # noqa: E402
from rayen_amd.constraint_module import ConstraintModule  # noqa: E402

PEAK_FP64 = 78.6e12
SHAPES = {"c2": dict(k=16, m=32, n_quad=2), "c3": dict(k=64, m=128, n_quad=4)}
LR = {"c2": 5e-4, "c3": 2e-5, "c5": 1e-5}      # with q ~ U(-0.25, 0.25) the reference iteration stays finite on every row
F64 = torch.float64


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def agree(t):
    return len(t) >= 2 and abs(t[-1] - t[-2]) <= 0.02 * t[-1]


def alternate(paths, reps, rounds, slow_ms):
    """{name: (ms, settled)}: the paths take turns, one window each a round, until every path's last two windows agree
    within 2 % (or ``rounds`` is reached)."""
    seen, reps = {name: [] for name in paths}, dict(reps)
    for name, fn in paths.items():
        first = window(fn, 1)                                  # (first call: allocations, images)
        if first > slow_ms:
            seen[name].append(first)
            reps[name] = 1
    for _ in range(rounds):
        for name, fn in paths.items():
            if not (reps[name] == 1 and seen[name] and agree(seen[name])):       # (a slow path stops once it has settled)
                seen[name].append(window(fn, reps[name]))
        if all(agree(t) for t in seen.values()):
            break
    return {name: (t[-1], agree(t)) for name, t in seen.items()}


def flops(n, m, nq, T):
    fwd = T * (4 * m * n + nq * (2 * n * n + 4 * n))
    bwd = (T - 1) * (4 * m * n + nq * (2 * n * n + 4 * n)) + T * (6 * m * n + nq * (4 * n * n + 8 * n))
    return fwd, fwd + bwd


def report(out, row):
    line = json.dumps(row)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def figures(row, res, new, old, per_row, B):
    for what, (a, b), fl in (("fwd", (new + "_fwd", old + "_fwd"), per_row[0]), ("fwd_bwd", (new + "_fb", old + "_fb"), per_row[1])):
        if a not in res or b not in res:
            row[f"{what}_not_measured"] = True
            continue
        row[f"{new}_{what}_ms"], row[f"{old}_{what}_ms"] = res[a][0], res[b][0]
        row[f"{what}_settled"] = bool(res[a][1] and res[b][1])
        row[f"{what}_{old}_over_{new}"] = res[b][0] / res[a][0]
        row[f"{new}_{what}_TFLOPs"] = B * fl / (res[a][0] * 1e-3) / 1e12
        row[f"{new}_{what}_share_of_fp64_matrix_peak"] = B * fl / (res[a][0] * 1e-3) / PEAK_FP64
    return row


def part_a(args, out):
    dev = torch.device("cuda:0")
    name = "c2"
    raw = workloads.random_lin_quad_soc(n_soc=0, seed=2, **SHAPES[name])
    dc3_args = dict(lr=LR[name], momentum=0.5, eps_converge=0.0, max_steps_training=args.steps, max_steps_testing=args.steps)
    layer = ConstraintModule(workloads.build_constraints(raw), method="DC3", create_map=False, args_DC3=dc3_args).to(dev)
    dp, _ = layer.dc3_pack(dev)
    n, k, B, T = dp.n, dp.k, args.batch, args.steps
    q = (torch.rand(B, n, device=dev, dtype=F64) * 2 - 1) * 0.25
    gy = torch.randn(B, k, device=dev, dtype=F64)
    lr, mom = LR[name], 0.5
    ys, steps = {}, None
    for kernel in ops.DC3_KERNELS_F64:
        ys[kernel], steps = ops.dc3_forward_raw(q, dp, lr, mom, 0.0, T, kernel=kernel)
        assert int(steps.item()) == T and torch.isfinite(ys[kernel]).all()
    err = float(((ys["tile64"] - ys["lane"]).abs().amax(dim=1) / ys["lane"].abs().amax(dim=1).clamp_min(1e-300)).max())

    def both(kernel):
        ops.dc3_backward_raw(q, ops.dc3_forward_raw(q, dp, lr, mom, 0.0, T, kernel=kernel)[1], gy, dp, lr, mom, T, kernel=kernel)

    paths = {"tile64_fwd": lambda: ops.dc3_forward_raw(q, dp, lr, mom, 0.0, T, kernel="tile64"),
             "lane_fwd": lambda: ops.dc3_forward_raw(q, dp, lr, mom, 0.0, T, kernel="lane"),
             "tile64_fb": lambda: both("tile64"), "lane_fb": lambda: both("lane")}
    res = alternate(paths, {p: args.reps for p in paths}, args.rounds, args.slow_ms)
    a = dc3.pack_arrays(layer)
    m, nq = a["A1e"].shape[0], a["Pe"].shape[0]
    report(out, figures({"part": "a", "set": name, "dtype": "fp64", "B": B, "n": n, "m": m, "nq": nq, "no": k - n, "steps": T,
                         "max_row_err_tile64_vs_lane": err}, res, "tile64", "lane", flops(n, m, nq, T), B))


def through_the_module(args, out, part, name, cs, batches):
    dev = torch.device("cuda:0")
    T = args.steps
    dc3_args = dict(lr=LR[name], momentum=0.5, eps_converge=0.0, max_steps_training=T, max_steps_testing=T, kernel="auto")
    layer = ConstraintModule(cs, method="DC3", create_map=False, args_DC3=dc3_args).to(dev).train()
    a = dc3.pack_arrays(layer)
    n, k, m, nq = a["n"], a["k"], a["A1e"].shape[0], a["Pe"].shape[0]
    dp, _ = layer.dc3_pack(dev)
    assert layer._dc3_kernel_for(dp, F64) == "tile64"
    for B in batches:
        q = ((torch.rand(B, n, 1, device=dev, dtype=F64) * 2 - 1) * 0.25)
        gy = torch.randn(B, k, 1, device=dev, dtype=F64)
        with torch.no_grad():
            y = layer(q)
            y_ref = layer._dc3_reference(q[:4096])
        assert layer.dc3_steps.tolist() == [T] and not layer._hip_unsupported and torch.isfinite(y).all()
        err = float(((y[:4096] - y_ref).abs().amax(dim=1) / y_ref.abs().amax(dim=1).clamp_min(1e-300)).max())
        del y, y_ref

        def fwd(route):
            with torch.no_grad():
                route(q)

        def both(route):
            leaf = q.detach().clone().requires_grad_(True)
            route(leaf).backward(gy)

        paths = {"tile64_fwd": lambda: fwd(layer), "eager_fwd": lambda: fwd(layer._dc3_reference),
                 "tile64_fb": lambda: both(layer)}
        if B <= args.eager_fb_max_batch:
            paths["eager_fb"] = lambda: both(layer._dc3_reference)
        reps = {p: (args.reps if p.startswith("tile64") else args.eager_reps) for p in paths}
        row = {"part": part, "set": name, "dtype": "fp64", "B": B, "n": n, "m": m, "nq": nq, "no": k - n, "steps": T,
               "max_row_err_tile64_vs_eager_first_4096_rows": err}
        try:
            res = alternate(paths, reps, args.eager_rounds, args.slow_ms)
        except torch.OutOfMemoryError as oom:                  # (the eager route's autograd graph at the large batch)
            report(out, dict(row, error="out of memory: " + str(oom)[:120]))
            continue
        report(out, figures(row, res, "tile64", "eager", flops(n, m, nq, T), B))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=262144, help="rows of parts (a) and (b)")
    ap.add_argument("--reps", type=int, default=5, help="calls in a window")
    ap.add_argument("--rounds", type=int, default=8, help="windows per path at the most, part (a)")
    ap.add_argument("--eager-reps", type=int, default=2)
    ap.add_argument("--eager-rounds", type=int, default=4, help="windows per path at the most, parts (b) and (c)")
    ap.add_argument("--slow-ms", type=float, default=5000.0, help="a path slower than this is timed one call a window")
    ap.add_argument("--eager-fb-max-batch", type=int, default=1 << 30,
                    help="beyond this batch the eager forward + backward is not timed (its row says so)")
    ap.add_argument("--c-batches", default="16384,262144", help="rows of part (c)")
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    report(out, {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "steps": args.steps, "dtype": "fp64",
                 "parts": args.parts, "method": "HIP events; alternating windows until two agree within 2 %"})
    parts = args.parts.split(",")
    if "a" in parts:
        part_a(args, out)
    if "b" in parts:
        raw = workloads.random_lin_quad_soc(n_soc=0, seed=2, **SHAPES["c3"])
        through_the_module(args, out, "b", "c3", workloads.build_constraints(raw), [args.batch])
    if "c" in parts:
        cs = workloads.build_constraints(workloads.make_raw("c5"))
        through_the_module(args, out, "c", "c5", cs, [int(b) for b in args.c_batches.split(",")])


if __name__ == "__main__":
    main()
