"""The fused wide forward (wide_kernel='fused', rayen_wide_fused.hip) against the products route (a library GEMM and
rayen_wide.hip over its products), fp32, forward through the module.

  lin1000   the reference sweep's k = 1000 with m = 1000 linear rows, B = 2 000
  qp500     k = 500 with 100 dense quadratics, B = 2 000
  mixed256  k = 256, m = 512, 4 quadratics, 2 cones, B = 262 144 (the products matrix is about 2 GB)

The protocol of scripts/bench_bar_stream.py: HIP events around timing windows of calls; a route is warm when two
consecutive timing windows agree within 2 %; every call takes the next of the rotating inputs (together larger than the
256 MiB Infinity Cache); both routes run in this process, alternating timing window by timing window.  Reported per route:
ms per call, useful TFLOP/s (2 B n rows of W_ext) against the 157.3 TFLOP/s fp32 MFMA peak, and the bytes the route moves by
its own design (not counters).  Lines go to stdout and are appended to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rayen_amd import _lib, workloads                           # noqa: E402
from rayen_amd.constraint_module import ConstraintModule        # noqa: E402

PEAK = 157.3e12            # fp32 MFMA, flop / s
DEV = "cuda:0"
SHAPES = {"lin1000": (dict(k=1000, m=1000, n_quad=0, n_soc=0, seed=1), 2000),
          "qp500": (dict(k=500, m=0, n_quad=100, n_soc=0, seed=2), 2000),
          "mixed256": (dict(k=256, m=512, n_quad=4, n_soc=2, seed=3), 262144)}


def window(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def warm(fn, calls, limit=12):
    prev = window(fn, calls)
    for n in range(limit):
        cur = window(fn, calls)
        if abs(cur - prev) <= 0.02 * prev:
            return n + 2
        prev = cur
    return -1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--calls", type=int, default=10, help="calls per timing window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "wide_fused.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide_fused.py measures on an MI355X; no HIP device here")
    os.environ["RAYEN_STRICT_HIP"] = "1"
    lines, record = [f"calls per timing window {args.calls}, timing windows {args.windows}"], {}
    for name in args.shapes.split(","):
        kw, B = SHAPES[name]
        t0 = time.time()
        cs = workloads.build_constraints(workloads.random_lin_quad_soc(**kw))
        layers = {"products": ConstraintModule(cs, create_map=False).to(DEV),
                  "fused": ConstraintModule(cs, create_map=False, wide_kernel="fused").to(DEV)}
        consts = layers["fused"].packed_constants()
        n, k = cs.n, cs.k
        rows = consts.W.shape[0] + (0 if consts.out_identity else k)
        count = max(2, -(-(600 << 20) // (B * n * 4)))
        xs = [torch.empty(B, n, 1, device=DEV).uniform_(-1, 1) for _ in range(count)]
        lines.append(f"{name}: n = {n}, k = {k}, {rows} rows of W_ext in {len(consts.segments)} segments, B = {B}, {count} rotating "
                     f"inputs of {B * n * 4 / 2 ** 20:.0f} MiB (setup {time.time() - t0:.1f} s)")
        turn = [0]
        paths = []
        for label, layer in layers.items():
            def run(layer=layer):
                i = turn[0] % len(xs)
                turn[0] += 1
                with torch.no_grad():
                    return layer(xs[i])
            y = run()
            kernel = _lib.load().rayen_last_forward_kernel()
            assert kernel == (_lib.KERNEL_WIDE_FUSED if label == "fused" else _lib.KERNEL_PRODUCTS), (label, kernel)
            paths.append((label, run, y))
        turn[0] = 0
        diff = float((layers["fused"](xs[0]) - layers["products"](xs[0])).abs().max())
        lines.append(f"    largest difference of the two routes' y on one input: {diff:.3e}")
        for label, run, _ in paths:
            lines.append(f"    {label}: warm after {warm(run, args.calls)} timing windows of {args.calls} calls")
        times = {label: [] for label, _, _ in paths}
        for _ in range(args.windows):
            for label, run, _ in paths:
                times[label].append(window(run, args.calls))
        flops = 2.0 * B * n * rows
        kp, rows_pad = (n + 7) // 8 * 8, (consts.W.shape[0] + 31) // 32 * 32 + (0 if consts.out_identity else (k + 31) // 32 * 32)
        moved = {"products": (f"v {B * n * 4 / 1e6:.0f} MB read twice, T {B * rows * 4 / 1e6:.0f} MB written and read, y "
                              f"{B * k * 4 / 1e6:.0f} MB written, W_ext {rows * n * 4 / 1e6:.1f} MB"),
                 "fused": (f"v {B * n * 4 / 1e6:.0f} MB read, y {B * k * 4 / 1e6:.0f} MB written"
                           + ("" if consts.out_identity else " and read back and rewritten")
                           + f", W_ext {rows_pad * kp * 4 / 1e6:.1f} MB from memory once and re-read from L2 by each of "
                           f"{-(-B // 32)} tiles ({-(-B // 32) * rows_pad * kp * 4 / 1e9:.1f} GB)")}
        for label, _, _ in paths:
            t = np.array(times[label])
            ms = float(np.median(t))
            lines.append(f"    {label}: median {ms:.4f} ms  min {t.min():.4f}  max {t.max():.4f}   useful "
                         f"{flops / (ms * 1e-3) / 1e12:.2f} TFLOP/s = {flops / (ms * 1e-3) / PEAK:.1%} of the fp32 MFMA peak")
            lines.append(f"        moves: {moved[label]}")
            record[f"{name}_{label}_ms"] = ms
        tf, tp = record[f"{name}_fused_ms"], record[f"{name}_products_ms"]
        lines.append(f"    fused against products: {tp / tf:.2f} x ({'fused faster' if tf < tp else 'fused NOT faster'})")
        del xs, layers, paths
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "wide_fused", **record}))


if __name__ == "__main__":
    main()
