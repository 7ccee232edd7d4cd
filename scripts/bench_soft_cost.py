"""Soft cost of config 3 (k = 64, 128 linear rows, 4 quadratics, 2 cones) at B = 262 144, fp32: loss + gradient per call.

  A  CostComputer(cs):              getSumSoftCostAllSamples(y).backward() in torch ops (the path before rayen_cost.hip)
  B  CostComputer(cs, fused=True):  the same call on rayen_amd::soft_cost -- one launch for loss and gradient
  K  the kernel alone (ops.soft_cost_raw with the gradient), for its share of the fp32 MFMA peak and its bytes

HIP events around windows of calls; a path is warm when two consecutive windows agree within 2 %; every call takes the
next of ROTATE input buffers (ROTATE x 64 MiB of y, beyond the 256 MiB cache), so y comes from HBM.  Both paths run in this
process, alternating windows.  Lines go to stdout and to profiles/bench/soft_cost_c3_fp32.txt (--out).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rayen_amd import ops, workloads                      # noqa: E402
from rayen_amd.cost_computer import CostComputer          # noqa: E402

PEAK_F32_MFMA = 157.3e12          # MI355X, v_mfma_f32_32x32x2_f32 (= the fp32 vector peak)
PEAK_HBM = 8.0e12


def window(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def warm(fn, calls, limit=20):
    prev = window(fn, calls)
    for n in range(limit):
        cur = window(fn, calls)
        if abs(cur - prev) <= 0.02 * prev:
            return n + 2
        prev = cur
    return -1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--calls", type=int, default=20, help="calls per window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=6)
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "soft_cost_c3_fp32.txt"))
    ap.add_argument("--only", default="", help="'B': the fused path alone (for a profiler run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_soft_cost.py measures on an MI355X; no HIP device here")

    cs = workloads.build_constraints(workloads.make_raw("c3", seed=0))
    B, k = args.batch, cs.k
    rng = np.random.default_rng(0)
    scale = torch.from_numpy(rng.choice([0.02, 0.3, 1.5], size=(B, 1))).float()
    ys = [((torch.rand((B, k), generator=torch.Generator().manual_seed(i)) * 2 - 1) * scale).cuda().unsqueeze(2)
          for i in range(args.rotate)]
    for y in ys:
        y.requires_grad_(True)
    turn = [0]

    def step(cc):
        def run():
            y = ys[turn[0] % len(ys)]
            turn[0] += 1
            y.grad = None
            cc.getSumSoftCostAllSamples(y).backward()
        return run

    plain, fused = CostComputer(cs).cuda(), CostComputer(cs, fused=True).cuda()
    pack, _ = fused.soft_cost.cost_pack(ys[0].device)

    def kernel():
        y = ys[turn[0] % len(ys)]
        turn[0] += 1
        ops.soft_cost_raw(y.detach()[:, :, 0], pack, True)

    paths = [("B fused=True", step(fused)), ("K kernel alone", kernel)]
    if args.only != "B":
        paths.insert(0, ("A torch ops", step(plain)))
    lines = [f"soft cost, config 3 (k={k}, rows 128 + 4 x 64 + 2 x 64), B={B}, fp32, loss + gradient; {args.windows} windows of "
             f"{args.calls} calls, {args.rotate} rotating inputs of {B * k * 4 / 2 ** 20:.0f} MiB"]
    times = {}
    for name, fn in paths:
        lines.append(f"{name}: warm after {warm(fn, args.calls)} windows")
    for _ in range(args.windows):                      # alternate the paths window by window
        for name, fn in paths:
            times.setdefault(name, []).append(window(fn, args.calls))
    for name, _ in paths:
        t = np.array(times[name])
        lines.append(f"{name}: median {np.median(t):.4f} ms  min {t.min():.4f}  max {t.max():.4f}")
    tk = float(np.median(times["K kernel alone"])) * 1e-3
    alg_bytes = 2 * B * k * 4 + 12 * B
    rows_first = 128 + 4 * 64 + 2 * 64
    rows_second = 128 + 2 * 64                           # the quadratics reuse P y
    flops = 2.0 * B * k * (rows_first + rows_second)
    lines.append(f"kernel: algorithmic bytes 2 B k 4 + 12 B = {alg_bytes / 1e6:.1f} MB -> {alg_bytes / tk / 1e12:.2f} TB/s "
                 f"({alg_bytes / tk / PEAK_HBM:.1%} of 8 TB/s); HBM counters not collected in this run")
    lines.append(f"kernel: {flops / 1e9:.1f} GFLOP on the matrix cores (first product {rows_first} rows, second {rows_second}) -> "
                 f"{flops / tk / 1e12:.1f} TFLOP/s = {flops / tk / PEAK_F32_MFMA:.1%} of the fp32 MFMA peak (157.3 TF): MFMA-bound")
    if "A torch ops" in times:
        ta, tb = float(np.median(times["A torch ops"])), float(np.median(times["B fused=True"]))
        lines.append(f"B against A: {ta / tb:.2f} x ({'B faster' if tb < ta else 'B NOT faster'})")
        # same numbers from both paths (fp32, different summation orders)
        y = ys[0]
        y.grad = None
        la = plain.getSumSoftCostAllSamples(y)
        la.backward()
        ga = y.grad.clone()
        y.grad = None
        lb = fused.getSumSoftCostAllSamples(y)
        lb.backward()
        lines.append(f"agreement: loss A {la.item():.6e} B {lb.item():.6e}; max |grad A - grad B| / max |grad A| = "
                     f"{float((ga - y.grad).abs().max() / ga.abs().max()):.2e}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "soft_cost_c3_fp32", "B": B, **{n: float(np.median(t)) for n, t in times.items()}}))


if __name__ == "__main__":
    main()
