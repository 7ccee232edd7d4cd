"""The fp64 fused wide backward (wide_backward='fused64', rayen_wide_fused_bwd64.hip) against the products route (two library
GEMMs around the coefficient kernel of rayen_wide.hip), fp64, on the four workloads of scripts/bench_wide_fused_bwd.py:

  lin1000    the reference sweep's k = 1000 with m = 1000 linear rows, B = 2 000
  qp500      k = 500 with 100 dense quadratics, B = 2 000
  qp500big   the same set, B = --big-batch (65 536: T and C of the products route are about 26 GB each in fp64)
  mixed256   k = 256, m = 512, 4 quadratics, 2 cones, B = 262 144 (T and C are about 4.3 GB each)

The protocol of scripts/bench_wide_fused_bwd.py: HIP events around timing windows of calls; a route is warm when two
consecutive timing windows agree within 2 %; every call takes the next of the rotating inputs (together larger than the
256 MiB Infinity Cache); every route runs in this process, alternating timing window by timing window.  Routes: 'products',
'fused64' (grouped by active constraint, the plan's tile), 'fused64' with group=False, and 'fused64' with the tile forced to
16 and to 32 samples (a forced 32 that the set's LDS plan does not serve is reported as such and left out).  Timed: the
backward alone (ops.backward_raw on recorded kappa and active) and forward + backward with each route's own forward
(wide_kernel='products' | 'fused64').  Reported per route: ms per call, the ratio to the products route, and the useful flop
of the fused route from the recorded active-segment histogram (2 n k per row for u = NA_E' g; 4 n r per row that a non-linear
segment of r rows clipped, and 4 n more for a cone's two aux rows) against the 78.6 TFLOP/s fp64 matrix peak.  Not measured:
hardware counters, the L2 hit rate of the re-reads of the images.  Lines go to stdout and are appended to --out.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_wide_fused import warm, window                       # noqa: E402
from bench_wide_fused_bwd import SHAPES                         # noqa: E402
from rayen_amd import _lib, ops, workloads                      # noqa: E402
from rayen_amd.constraint_module import ConstraintModule        # noqa: E402

DEV = "cuda:0"
PEAK_FP64 = 78.6e12        # fp64 MFMA, flop / s
ROUTES = {"products": dict(wide_backward="products"),
          "fused64": dict(wide_backward="fused64"),
          "fused64, group=False": dict(wide_backward="fused64", group=False),
          "fused64, 16 samples": dict(wide_backward="fused64", wide_samples=16),
          "fused64, 32 samples": dict(wide_backward="fused64", wide_samples=32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--calls", type=int, default=5, help="calls per timing window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--big-batch", type=int, default=65536, help="B of qp500big")
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "wide_fused_bwd64.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide_fused_bwd64.py measures on an MI355X; no HIP device here")
    os.environ["RAYEN_STRICT_HIP"] = "1"
    torch.set_default_dtype(torch.float64)
    lib = _lib.load()
    lines, record = [f"fp64; calls per timing window {args.calls}, timing windows {args.windows}"], {}
    cache = {}
    for name in args.shapes.split(","):
        kw, B = SHAPES[name]
        if name == "qp500big":
            B = args.big_batch
        t0 = time.time()
        key = json.dumps(kw, sort_keys=True)
        if key not in cache:
            cache.clear()
            cs = workloads.build_constraints(workloads.random_lin_quad_soc(**kw))
            cache[key] = (cs, ConstraintModule(cs, create_map=False).to(DEV))
        cs, layer = cache[key]
        dp = layer.device_pack(torch.device(DEV))[0]
        consts = layer.packed_constants()
        n, k = cs.n, cs.k
        rows = consts.W.shape[0] + (0 if consts.out_identity else k)
        plan = np.zeros(11, dtype=np.int64)
        served32 = (lib.rayen_wide_fused_bwd64_plan(dp.handle, 32, plan.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == 0
                    and int(plan[10]) == 1)
        lib.rayen_wide_fused_bwd64_plan(dp.handle, 0, plan.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        routes = [r for r in ROUTES if served32 or r != "fused64, 32 samples"]
        count = max(2, -(-(600 << 20) // (B * n * 8)))
        sets = []
        for _ in range(count):
            v = torch.empty(B, n, device=DEV).uniform_(-1, 1)
            _, kappa, active = ops.project_raw(v, dp, wide_kernel="fused64")
            sets.append((v, kappa, active, torch.empty(B, k, device=DEV).uniform_(-1, 1)))
        # the recorded histogram of the first input: rows by active segment, the fused route's useful flop
        kap, act = sets[0][1].cpu().numpy(), sets[0][2].cpu().numpy()
        clipped = kap > 1
        useful = 0.0 if consts.out_identity else 2.0 * B * n * k
        hist = {}
        for i, s in enumerate(consts.segments):
            rows_of = int(np.sum(clipped & (act[:, 0] == i)))
            if rows_of:
                hist[i] = rows_of
            if s.type != _lib.SEG_LIN:
                useful += rows_of * (4.0 * n * s.nrows + (4.0 * n if s.type == _lib.SEG_SOC else 0.0))
        nonlinear = sum(c for i, c in hist.items() if consts.segments[i].type != _lib.SEG_LIN)
        lines.append(f"{name}: n = {n}, k = {k}, {rows} rows of W_ext in {len(consts.segments)} segments, B = {B}, {count} rotating "
                     f"inputs (setup {time.time() - t0:.1f} s)")
        lines.append(f"    clipped rows {int(clipped.sum())}, by a non-linear segment {nonlinear} ({len(hist)} distinct active "
                     f"segments); products route 4 B n rows = {4.0 * B * n * rows / 1e12:.3f} Tflop and two [B, rows] fp64 matrices of "
                     f"{8.0 * B * rows / 1e9:.2f} GB each, fused route useful {useful / 1e12:.4f} Tflop; the plan's tile "
                     f"{int(plan[7])} samples, {int(plan[9])} bytes of LDS, a forced 32 {'served' if served32 else 'not served'}; "
                     f"grouping workspace {lib.rayen_wide_fused_bwd64_workspace_bytes(dp.handle, B)} bytes")
        turn = [0]

        def bwd(route):
            v, kappa, active, G = sets[turn[0] % len(sets)]
            turn[0] += 1
            return ops.backward_raw(v, kappa, active, G, dp, **ROUTES[route])

        def both(route):
            v, _, _, G = sets[turn[0] % len(sets)]
            turn[0] += 1
            _, kappa, active = ops.project_raw(v, dp, wide_kernel="products" if route == "products" else "fused64")
            return ops.backward_raw(v, kappa, active, G, dp, **ROUTES[route])

        turn[0] = 0
        ref = bwd("products")
        turn[0] = 0
        got = bwd("fused64")
        diff = float((got - ref).abs().max() / ref.abs().max())
        lines.append(f"    largest difference of the two routes' grad_v on one input, against the largest entry: {diff:.3e}")
        del ref, got
        for what, fn in (("backward", bwd), ("forward + backward", both)):
            for route in routes:
                w = warm(lambda: fn(route), args.calls)
                lines.append(f"    {what}, {route}: warm after {w} timing windows of {args.calls} calls")
            times = {route: [] for route in routes}
            for _ in range(args.windows):
                for route in routes:
                    times[route].append(window(lambda: fn(route), args.calls))
            for route in routes:
                t = np.array(times[route])
                ms = float(np.median(t))
                record[f"{name}_{what.replace(' + ', '_')}_{route.replace(', ', '_').replace(' ', '_').replace('=', '_')}_ms"] = ms
                extra = ""
                if route != "products" and what == "backward":
                    extra = (f"   useful {useful / (ms * 1e-3) / 1e12:.2f} TFLOP/s = {useful / (ms * 1e-3) / PEAK_FP64:.1%} of the fp64 "
                             "matrix peak")
                base = float(np.median(times["products"]))
                lines.append(f"    {what}, {route}: median {ms:.4f} ms  min {t.min():.4f}  max {t.max():.4f}   products / this = "
                             f"{base / ms:.2f} x{extra}")
        del sets
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "wide_fused_bwd64", **record}))


if __name__ == "__main__":
    main()
