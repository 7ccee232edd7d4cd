"""Euclidean projection onto sets with an LMI (``ProjectionModule(..., lmi=True)``), fp32: the torch mirror on the device
against the kernel.

  M  projection.mirror_forward / mirror_backward on the device: the same iteration in torch ops, ``torch.linalg.eigh`` (the
     vendor solver) on the whole batch once per iteration
  K  rayen_amd::euclid_project on rayen_proj.hip: one wave per sample, parallel cyclic Jacobi in LDS once per iteration

on config 4's shape (k = 10, 20 x 20, B = 16 384) and a small one (k = 6, 8 x 8, B = 16 384), forward alone and forward +
backward, both paths at the same ``--max-iters`` and ``eps`` (rows that need more stop at the limit on both paths; the mean
iterations per row are reported).  HIP events around windows of calls; a path is warm when two consecutive windows agree
within 2 %.  Both paths run in this process, alternating windows.  Lines go to stdout and to profiles/bench/proj_lmi.txt
(--out).  No ratio is expected in advance; no hardware counters are collected here.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rayen_amd import projection, workloads                # noqa: E402


def window(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def warm(fn, calls, limit):
    prev = window(fn, calls)
    for n in range(limit):
        cur = window(fn, calls)
        if abs(cur - prev) <= 0.02 * prev:
            return n + 2
        prev = cur
    return -1


# name -> (raw set, rho (None: build_program probes for it; config 4's probing takes a minute and chose 10), batch)
WORKLOADS = {
    "c4 shape (k=10, 20x20)": (lambda: workloads.random_lmi(10, 20, seed=0), 10.0, 16384),
    "small (k=6, 8x8)": (lambda: workloads.random_lmi(6, 8, seed=0), None, 16384),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--warm-limit", type=int, default=4)
    ap.add_argument("--max-iters", type=int, default=64)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--amp", type=float, default=1.5)
    ap.add_argument("--batch", type=int, default=0, help="override the batch of every workload")
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "proj_lmi.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_proj_lmi.py measures on an MI355X; no HIP device here")

    lines, result = [], {"bench": "proj_lmi"}
    for name, (make, rho, B) in WORKLOADS.items():
        B = args.batch or B
        cs = workloads.build_constraints(make())
        layer = projection.ProjectionModule(cs, create_map=False, lmi=True, rho=rho, max_iters=args.max_iters,
                                            eps=args.eps).cuda()
        rng = np.random.default_rng(0)
        q = cs.z0.reshape(1, -1) + args.amp * rng.uniform(0.0, 1.5, (B, 1)) * rng.standard_normal((B, cs.n))
        q = torch.from_numpy(q).float().cuda()
        g = torch.from_numpy(rng.standard_normal((B, cs.n))).float().cuda()
        c = layer.constants(torch.float32, q.device)

        def mirror_fwd():
            return projection.mirror_forward(c, q, args.max_iters, args.eps)

        def mirror_both():
            z, iters, vstar = mirror_fwd()
            return projection.mirror_backward(c, g, vstar, iters, args.max_iters, args.eps)

        def kernel_fwd():
            with torch.no_grad():
                return layer.project(q)

        def kernel_both():
            qg = q.detach().requires_grad_(True)
            z, _ = layer.project(qg)
            z.backward(g)
            return qg.grad

        zk, ik = kernel_fwd()
        zm, im, _ = mirror_fwd()
        assert layer._proj_packs and not layer._unsupported          # (K ran on the kernel)
        lines.append(f"projection onto an LMI set, {name}, B={B}, fp32, rho={layer.program.rho:g}, max_iters={args.max_iters}, "
                     f"eps={args.eps:g}; {args.windows} windows of {args.calls} calls")
        lines.append(f"  iterations per row: K mean {float(ik.float().mean()):.1f} max {int(ik.max())}; M mean "
                     f"{float(im.float().mean()):.1f} max {int(im.max())}; {float((ik == 0).float().mean()):.0%} of the rows inside, "
                     f"{float((ik == args.max_iters).float().mean()):.0%} at the limit")
        gm, gk = mirror_both(), kernel_both()
        lines.append(f"  agreement: max |z M - z K| / (1 + max |z|) = {float((zm - zk).abs().max() / (1 + zm.abs().max())):.2e}; "
                     f"max |grad M - grad K| / (1 + max |grad|) = {float((gm - gk).abs().max() / (1 + gm.abs().max())):.2e}")
        for what, pm, pk in (("forward", mirror_fwd, kernel_fwd), ("forward + backward", mirror_both, kernel_both)):
            paths = [("M mirror", pm), ("K kernel", pk)]
            times = {}
            for label, fn in paths:
                lines.append(f"  {what}, {label}: warm after {warm(fn, args.calls, args.warm_limit)} windows")
            for _ in range(args.windows):                      # alternate the paths window by window
                for label, fn in paths:
                    times.setdefault(label, []).append(window(fn, args.calls))
            for label, _ in paths:
                t = np.array(times[label])
                lines.append(f"  {what}, {label}: median {np.median(t):.3f} ms  min {t.min():.3f}  max {t.max():.3f}")
            tm, tk = float(np.median(times["M mirror"])), float(np.median(times["K kernel"]))
            lines.append(f"  {what}, K against M: {tm / tk:.2f} x ({'K faster' if tk < tm else 'K NOT faster: the kernel loses to the mirror here'})")
            result[f"{name} {what}"] = {"mirror_ms": tm, "kernel_ms": tk}
        print("\n".join(lines[-12:]), flush=True)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
