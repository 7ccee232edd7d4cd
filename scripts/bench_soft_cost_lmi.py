"""Soft cost of sets with an LMI, fp32, loss + gradient per call: the torch mirror against the kernel.

  M  soft_cost.mirror(...).sum().backward(): einsum -> [B, r, r], torch.linalg.eigvalsh (the vendor solver), autograd
  K  SoftCost(cs)(y).sum().backward() on rayen_amd::soft_cost: rayen_cost_lmi.hip (after rayen_cost.hip on the mixed set)

on three workloads: config 4 (k = 10, 20 x 20, B = 16 384), the r = 100 point of the reference's LMI sweep (k = 100,
B = 2 000) and a mixed set (32 linear rows + a 20 x 20 LMI, k = 10, B = 16 384).

HIP events around windows of calls; a path is warm when two consecutive windows agree within 2 %; every call takes the next
of ROTATE input buffers.  Both paths run in this process, alternating windows.  Lines go to stdout and to
profiles/bench/soft_cost_lmi.txt (--out).  No ratio is expected in advance: a wave per sample keeps 20 of its 64 lanes busy
at r = 20.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rayen_amd import soft_cost, workloads                # noqa: E402
from rayen_amd.soft_cost import SoftCost                  # noqa: E402


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


def mixed_raw():
    raw = workloads.random_lmi(10, 20, seed=0)
    rng = np.random.default_rng(1)
    raw["A1"], raw["b1"] = rng.uniform(-1.0, 1.0, size=(32, 10)), rng.uniform(0.1, 1.0, size=(32, 1))
    return raw


# name -> (raw set, batch, calls per window)
WORKLOADS = {
    "c4 (k=10, 20x20)": (lambda: workloads.make_raw("c4", seed=0), 16384, 10),
    "sweep r=100 (k=100, 100x100)": (lambda: workloads.random_lmi(100, 100, seed=0), 2000, 2),
    "mixed (32 linear rows + 20x20, k=10)": (mixed_raw, 16384, 10),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--warm-limit", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "soft_cost_lmi.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_soft_cost_lmi.py measures on an MI355X; no HIP device here")

    lines, result = [], {"bench": "soft_cost_lmi"}
    for name, (make, B, calls) in WORKLOADS.items():
        cs = workloads.build_constraints(make())
        k = cs.k
        sc = SoftCost(cs).cuda()
        rng = np.random.default_rng(0)
        scale = torch.from_numpy(rng.choice([0.02, 0.3, 1.5], size=(B, 1))).float()
        ys = [((torch.rand((B, k), generator=torch.Generator().manual_seed(i)) * 2 - 1) * scale).cuda().requires_grad_(True)
              for i in range(args.rotate)]
        turn = [0]
        consts = sc.constants(torch.float32, ys[0].device)

        def next_y():
            y = ys[turn[0] % len(ys)]
            turn[0] += 1
            y.grad = None
            return y

        def run_mirror():
            soft_cost.mirror(consts, next_y())[0].sum().backward()

        def run_kernel():
            sc(next_y()).sum().backward()

        paths = [("M mirror", run_mirror), ("K kernel", run_kernel)]
        lines.append(f"soft cost, {name}, B={B}, fp32, loss + gradient; {args.windows} windows of {calls} calls, "
                     f"{args.rotate} rotating inputs")
        times = {}
        for label, fn in paths:
            lines.append(f"  {label}: warm after {warm(fn, calls, args.warm_limit)} windows")
        for _ in range(args.windows):                      # alternate the paths window by window
            for label, fn in paths:
                times.setdefault(label, []).append(window(fn, calls))
        for label, _ in paths:
            t = np.array(times[label])
            lines.append(f"  {label}: median {np.median(t):.4f} ms  min {t.min():.4f}  max {t.max():.4f}")
        tm, tk = float(np.median(times["M mirror"])), float(np.median(times["K kernel"]))
        lines.append(f"  K against M: {tm / tk:.2f} x ({'K faster' if tk < tm else 'K NOT faster: the kernel loses to the mirror here'})")
        assert sc._cost_packs and not sc._unsupported      # (K ran on the kernel)
        # the same numbers from both paths
        y = next_y()
        cm = soft_cost.mirror(consts, y)[0]
        cm.sum().backward()
        gm = y.grad.clone()
        y.grad = None
        ck = sc(y)
        ck.sum().backward()
        cm, ck = cm.detach(), ck.detach()
        outside = float((cm > 0).float().mean())
        lines.append(f"  agreement: max |cost M - cost K| / max cost = {float((cm - ck).abs().max() / cm.abs().max()):.2e}; "
                     f"max |grad M - grad K| / max |grad M| = {float((gm - y.grad).abs().max() / gm.abs().max()):.2e}; "
                     f"{outside:.0%} of the rows outside the set")
        result[name] = {"mirror_ms": tm, "kernel_ms": tk}
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
