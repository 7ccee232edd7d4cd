#!/usr/bin/env python
"""Time method='DC3' (rayen_amd/csrc/rayen_dc3.hip) forward and backward with HIP events, next to the reference's
iteration in eager torch ops on the same GPU (``ConstraintModule._dc3_reference`` and autograd through it).

    python scripts/dc3_bench.py [--reps 10] [--batch 262144] [--steps 10] [--sets c2,c3]

The sets are the linear-plus-quadratic parts of configs 2 and 3 (config 3's cones dropped).  ``eps_converge = 0`` pins the
step count to ``--steps`` on both sides.  Flops per row and step: 4 m n (two passes over A1e) + nq (2 n^2 + 4 n) forward; the
fraction is against the 157.3 TFLOP/s fp32 vector peak of the MI355X.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rayen_amd import ops, workloads  # noqa: E402
from rayen_amd.constraint_module import ConstraintModule  # noqa: E402

PEAK_FP32_VECTOR = 157.3e12
SHAPES = {"c2": dict(k=16, m=32, n_quad=2), "c3": dict(k=64, m=128, n_quad=4)}
LR = {"c2": 5e-4, "c3": 2e-5}      # with q ~ U(-0.25, 0.25) the reference iteration stays finite on every row


def time_call(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sets", default="c2,c3")
    ap.add_argument("--eager-batch", type=int, default=0, help="rows of the eager comparator (0: the full batch, what a "
                    "recorded number must use); a smaller one is scaled linearly, which OVERSTATES the eager time "
                    "(launch overhead dominates small batches) and is marked in the output")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.sets.split(","):
        shape = SHAPES[name]
        raw = workloads.random_lin_quad_soc(n_soc=0, seed=2, **shape)
        dc3_args = dict(lr=LR[name], momentum=0.5, eps_converge=0.0, max_steps_training=args.steps,
                        max_steps_testing=args.steps)
        layer = ConstraintModule(workloads.build_constraints(raw), method="DC3", create_map=False, args_DC3=dc3_args).to(dev)
        layer.train()
        n, k, m, nq = layer.n, layer.k, shape["m"], shape["n_quad"]
        B = args.batch
        dp, _ = layer.dc3_pack(dev)
        q = (torch.rand(B, n, device=dev) * 2 - 1) * 0.25
        gy = torch.randn(B, k, device=dev)
        lr, mom = dc3_args["lr"], 0.5
        y, steps = ops.dc3_forward_raw(q, dp, lr, mom, 0.0, args.steps)
        assert int(steps.item()) == args.steps and torch.isfinite(y).all()
        fwd = time_call(lambda: ops.dc3_forward_raw(q, dp, lr, mom, 0.0, args.steps), args.reps)
        bwd = time_call(lambda: ops.dc3_backward_raw(q, steps, gy, dp, lr, mom, args.steps), args.reps)
        Be = args.eager_batch or B
        qe = q[:Be].unsqueeze(2)
        with torch.no_grad():
            y_ref = layer._dc3_reference(qe)[:, :, 0]
            eager_fwd = time_call(lambda: layer._dc3_reference(qe), max(3, args.reps // 2)) * (B / Be)
        err = float(((y[:Be] - y_ref).abs().amax(dim=1) / y_ref.abs().amax(dim=1).clamp_min(1e-30)).max())

        def eager_both():
            leaf = qe.detach().clone().requires_grad_(True)
            layer._dc3_reference(leaf)[:, :, 0].backward(gy[:Be])

        eager_fb = time_call(eager_both, max(3, args.reps // 2)) * (B / Be)
        flops = B * args.steps * (4 * m * n + nq * (2 * n * n + 4 * n))
        print(json.dumps({"set": name, "B": B, "n": n, "m": m, "n_quad": nq, "steps": args.steps,
                          "fwd_ms": fwd * 1e3, "bwd_ms": bwd * 1e3, "eager_fwd_ms": eager_fwd * 1e3,
                          "eager_fwd_bwd_ms": eager_fb * 1e3, "eager_rows": Be, "eager_scaled": Be != B,
                          "fwd_speedup": eager_fwd / fwd, "fwd_bwd_speedup": eager_fb / (fwd + bwd),
                          "fwd_TFLOPs": flops / fwd / 1e12, "fwd_frac_fp32_vector_peak": flops / fwd / PEAK_FP32_VECTOR,
                          "max_row_err_vs_eager": err}), flush=True)


if __name__ == "__main__":
    main()
