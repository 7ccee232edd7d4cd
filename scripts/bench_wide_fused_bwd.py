"""The fused wide backward (wide_backward='fused', rayen_wide_fused_bwd.hip) against the products route (two library GEMMs
around the coefficient kernel of rayen_wide.hip), fp32.

  lin1000    the reference sweep's k = 1000 with m = 1000 linear rows, B = 2 000
  qp500      k = 500 with 100 dense quadratics, B = 2 000
  qp500big   the same set, B = 65 536
  mixed256   k = 256, m = 512, 4 quadratics, 2 cones, B = 262 144 (T and C of the products route are about 2 GB each)

The protocol of scripts/bench_wide_fused.py: HIP events around timing windows of calls; a route is warm when two consecutive
timing windows agree within 2 %; every call takes the next of the rotating inputs (together larger than the 256 MiB Infinity
Cache); 'products', 'fused' (grouped by active constraint) and 'fused' with group=False run in this process, alternating
timing window by timing window.  Timed: the backward alone (ops.backward_raw on recorded kappa and active) and forward +
backward (ops.project_raw with the route's own forward, then the backward).  Reported per route: ms per call, the ratio to
the products route, the useful flop of the fused route from the recorded active-segment histogram (2 n k per row for
u = NA_E' g; 4 n r per row that a non-linear segment of r rows clipped, and 4 n more for a cone's two aux rows) against the
157.3 TFLOP/s fp32 MFMA peak, and the cost of the grouping launches (grouped against group=False on a batch that is
already sorted by key: the same tiles either way).  Lines go to stdout and are appended to --out.
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

from bench_wide_fused import PEAK, warm, window                 # noqa: E402
from rayen_amd import _lib, ops, workloads                      # noqa: E402
from rayen_amd.constraint_module import ConstraintModule        # noqa: E402

DEV = "cuda:0"
SHAPES = {"lin1000": (dict(k=1000, m=1000, n_quad=0, n_soc=0, seed=1), 2000),
          "qp500": (dict(k=500, m=0, n_quad=100, n_soc=0, seed=2), 2000),
          "qp500big": (dict(k=500, m=0, n_quad=100, n_soc=0, seed=2), 65536),
          "mixed256": (dict(k=256, m=512, n_quad=4, n_soc=2, seed=3), 262144)}
ROUTES = {"products": dict(wide_backward="products"), "fused": dict(wide_backward="fused"),
          "fused, group=False": dict(wide_backward="fused", group=False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--calls", type=int, default=5, help="calls per timing window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "wide_fused_bwd.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide_fused_bwd.py measures on an MI355X; no HIP device here")
    os.environ["RAYEN_STRICT_HIP"] = "1"
    lines, record = [f"calls per timing window {args.calls}, timing windows {args.windows}"], {}
    cache = {}
    for name in args.shapes.split(","):
        kw, B = SHAPES[name]
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
        count = max(2, -(-(600 << 20) // (B * n * 4)))
        sets = []
        for _ in range(count):
            v = torch.empty(B, n, device=DEV).uniform_(-1, 1)
            _, kappa, active = ops.project_raw(v, dp, wide_kernel="fused")
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
                     f"segments); products route 4 B n rows = {4.0 * B * n * rows / 1e12:.3f} Tflop, fused route useful "
                     f"{useful / 1e12:.4f} Tflop; grouping workspace "
                     f"{_lib.load().rayen_wide_fused_bwd_workspace_bytes(dp.handle, B)} bytes")
        turn = [0]

        def bwd(route, data=sets):
            v, kappa, active, G = data[turn[0] % len(data)]
            turn[0] += 1
            return ops.backward_raw(v, kappa, active, G, dp, **ROUTES[route])

        def both(route):
            v, _, _, G = sets[turn[0] % len(sets)]
            turn[0] += 1
            _, kappa, active = ops.project_raw(v, dp, wide_kernel="products" if route == "products" else "fused")
            return ops.backward_raw(v, kappa, active, G, dp, **ROUTES[route])

        turn[0] = 0
        ref = bwd("products")
        turn[0] = 0
        got = bwd("fused")
        diff = float((got - ref).abs().max() / ref.abs().max())
        lines.append(f"    largest difference of the two routes' grad_v on one input, against the largest entry: {diff:.3e}")
        del ref, got
        for what, fn in (("backward", bwd), ("forward + backward", both)):
            for route in ROUTES:
                w = warm(lambda: fn(route), args.calls)
                lines.append(f"    {what}, {route}: warm after {w} timing windows of {args.calls} calls")
            times = {route: [] for route in ROUTES}
            for _ in range(args.windows):
                for route in ROUTES:
                    times[route].append(window(lambda: fn(route), args.calls))
            for route in ROUTES:
                t = np.array(times[route])
                ms = float(np.median(t))
                record[f"{name}_{what.replace(' + ', '_')}_{route.replace(', group=False', '_ungrouped')}_ms"] = ms
                extra = ""
                if route != "products" and what == "backward":
                    extra = (f"   useful {useful / (ms * 1e-3) / 1e12:.2f} TFLOP/s = {useful / (ms * 1e-3) / PEAK:.1%} of the fp32 "
                             "MFMA peak")
                base = float(np.median(times["products"]))
                lines.append(f"    {what}, {route}: median {ms:.4f} ms  min {t.min():.4f}  max {t.max():.4f}   products / this = "
                             f"{base / ms:.2f} x{extra}")
        # the grouping launches alone: a batch already sorted by key walks the same tiles grouped or not
        v, kappa, active, G = sets[0]
        nl = torch.tensor([0 if s.type == _lib.SEG_LIN else 1 + i for i, s in enumerate(consts.segments)], device=DEV)
        keys = torch.where((kappa > 1) & (active[:, 0] >= 0), nl[active[:, 0].clamp_min(0).long()], torch.zeros_like(nl[:1]))
        order = torch.argsort(keys, stable=True)
        srt = [tuple(t[order].contiguous() for t in (v, kappa, active, G))]
        t_sorted = {}
        for route in ("fused", "fused, group=False"):
            warm(lambda: bwd(route, srt), args.calls)
        for _ in range(args.windows):
            for route in ("fused", "fused, group=False"):
                t_sorted.setdefault(route, []).append(window(lambda: bwd(route, srt), args.calls))
        tg, tu = (float(np.median(t_sorted[r])) for r in ("fused", "fused, group=False"))
        lines.append(f"    on a batch already sorted by key (one input, cache-warm): grouped {tg:.4f} ms, group=False {tu:.4f} ms: "
                     f"the grouping launches cost {tg - tu:.4f} ms")
        record[f"{name}_grouping_ms"] = tg - tu
        del sets, srt
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "wide_fused_bwd", **record}))


if __name__ == "__main__":
    main()
