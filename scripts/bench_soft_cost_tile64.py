"""The fp64 tile soft cost (rayen_cost_tile64.hip, kernel='tile64') against what served its sets before, all in fp64:

  (a) config 3 (k = 64, 128 linear rows, 4 quadratics, 2 cones), B = 262 144, loss + gradient:
      T  SoftCost(cs, kernel='tile64')    against    S  kernel='stream' (the lane kernel, streamed)  and  M  the mirror
  (b) config 5 (k = 45, ~1.1 k corridor rows, 72 quadratics, 15 equalities), B = 262 144 and 16 384, loss + gradient:  T against S
  (c) config 2 (k = 16, 32 linear rows, 2 quadratics), B = 262 144, loss + gradient:  T against R  the resident lane kernel
  (d) config 3, B = 262 144, values only (no gradient asked for: grad = NULL in the library):  T against S

The protocol of scripts/bench_soft_cost_stream.py: HIP events around timing windows of calls (not to be confused with the
windows the image is cut into); a path is warm when two consecutive timing windows agree within 2 %; every call takes the next
of ROTATE input buffers (together beyond the Infinity Cache); the paths of a row run in this process, alternating timing
window by timing window -- "before" is the other route measured here, never a figure from a document.  A call is
``cost = module(y); cost.sum().backward()`` (rows a - c) or ``module(y)`` under ``torch.no_grad()`` (row d).  No ratio is a
pass condition.  Lines go to stdout and to profiles/bench/soft_cost_tile64.txt (--out).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import PEAK_FP64_TFLOPS                        # noqa: E402
from rayen_amd import workloads                           # noqa: E402
from rayen_amd.soft_cost import SoftCost                  # noqa: E402

# row -> (config, batches, the other routes, loss + gradient?)
ROWS = {"a": ("c3", (262144,), ("stream", "mirror"), True), "b": ("c5", (262144, 16384), ("stream",), True),
        "c": ("c2", (262144,), ("resident",), True), "d": ("c3", (262144,), ("stream",), False)}
TAGS = {"tile64": "T tile64", "stream": "S stream", "resident": "R resident", "mirror": "M mirror"}


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


def blocks(a):
    """(blocks of the first product, blocks of the second product) of the tile image: a quadratic's gradient reuses P y."""
    up = lambda n: -(-n // 16)          # noqa: E731
    lin = up(a["b1"].size) + up(a["b2"].size)
    cones = sum(up(int(r)) for r in a["soc_rows"])
    return lin + up(a["k"]) * a["r"].size + cones, lin + cones


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="a,b,c,d")
    ap.add_argument("--calls", type=int, default=10, help="calls per timing window (the mirror: a fifth of it, at least 2)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=6)
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "soft_cost_tile64.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_soft_cost_tile64.py measures on an MI355X; no HIP device here")
    os.environ.pop("RAYEN_STRICT_HIP", None)          # (the mirror is one of the paths)
    lines, record, sets = [], {}, {}
    for row in args.rows.split(","):
        config, batches, others, with_grad = ROWS[row]
        if config not in sets:
            sets[config] = workloads.build_constraints(workloads.make_raw(config, seed=0))
        cs = sets[config]
        k = cs.k
        modules = {"tile64": SoftCost(cs, kernel="tile64").cuda(), "stream": SoftCost(cs, kernel="stream").cuda(),
                   "resident": SoftCost(cs).cuda()}
        modules["mirror"] = modules["resident"]          # (config 3 in fp64: the default module refuses, loudly, and runs the mirror)
        a = modules["tile64"].arrays
        for B in batches:
            rng = np.random.default_rng(0)
            y0 = torch.from_numpy(np.asarray(cs.y0, dtype=np.float64).reshape(1, k))
            span = 1.0 + float(y0.abs().max())
            scale = torch.from_numpy(rng.choice([0.02, 0.3, 1.5], size=(B, 1)))
            ys = [(y0 + span * (torch.rand((B, k), dtype=torch.float64, generator=torch.Generator().manual_seed(i)) * 2 - 1) * scale)
                  .cuda().requires_grad_(with_grad) for i in range(args.rotate)]
            turn = [0]

            def step(module):
                def run():
                    y = ys[turn[0] % len(ys)]
                    turn[0] += 1
                    if with_grad:
                        y.grad = None
                        module(y).sum().backward()
                    else:
                        with torch.no_grad():
                            module(y)
                return run

            pack, _ = modules["tile64"].cost_pack(ys[0].device)
            assert pack.tile64_served()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                modules["resident"](ys[0].detach())
            assert bool(modules["resident"]._unsupported) == ("resident" not in others), "the row names the wrong 'before' route"
            paths = [(TAGS[r], step(modules[r]), max(args.calls // 5, 2) if r == "mirror" else args.calls) for r in ("tile64",) + others]
            name = f"({row}) {config} float64 B={B} {'loss + gradient' if with_grad else 'values only'}"
            first, second = blocks(a)
            K = 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64
            image = (first * (16 * K + 21) + (a["r"].size + a["soc_rows"].size) * max(K, 16)) * 8
            lines.append(f"{name}: k={k}, rows {a['b1'].size} + {a['r'].size} quadratics + {a['soc_rows'].size} cones + {a['b2'].size} "
                         f"equalities; tile image {image / 1024:.0f} KiB in {first} blocks (K = {K}); {args.windows} timing windows, "
                         f"{args.rotate} rotating inputs of {B * k * 8 / 2 ** 20:.0f} MiB")
            times = {}
            for label, fn, calls in paths:
                lines.append(f"  {label}: warm after {warm(fn, calls)} timing windows of {calls} calls")
            for _ in range(args.windows):
                for label, fn, calls in paths:
                    times.setdefault(label, []).append(window(fn, calls))
            med = {}
            for label, _, _ in paths:
                t = np.array(times[label])
                med[label] = float(np.median(t))
                lines.append(f"  {label}: median {np.median(t):.4f} ms  min {t.min():.4f}  max {t.max():.4f}")
            tt = med[TAGS["tile64"]]
            for r in others:
                verdict = "T faster" if tt < med[TAGS[r]] else "T NOT faster"
                lines.append(f"  T against {TAGS[r][0]}: {med[TAGS[r]] / tt:.2f} x ({verdict})")
            rows_lin = a["b1"].size + a["b2"].size + int(a["soc_rows"].sum())
            useful = 2.0 * B * k * (rows_lin * (2 if with_grad else 1) + a["r"].size * k)
            executed = 2.0 * B * 16 * K * (first + (second if with_grad else 0))
            lines.append(f"  T: {useful / 1e9:.1f} useful GFLOP ({executed / 1e9:.1f} executed in whole blocks when every second product "
                         f"runs) -> {useful / (tt * 1e-3) / 1e12:.2f} useful TFLOP/s = {useful / (tt * 1e-3) / 1e12 / PEAK_FP64_TFLOPS:.1%} of "
                         f"the fp64 peak ({PEAK_FP64_TFLOPS} TF), the module's host work"
                         + (" and backward multiply included" if with_grad else " included"))
            # the same numbers from every path
            outs = {}
            for r in ("tile64",) + others:
                y = ys[0]
                if with_grad:
                    y.grad = None
                    cost = modules[r](y)
                    cost.sum().backward()
                    outs[r] = (cost.detach(), y.grad.clone())
                else:
                    with torch.no_grad():
                        outs[r] = (modules[r](y), None)
            for r in others:
                (ct, gt), (co, go) = outs["tile64"], outs[r]
                line = f"  agreement: max |cost T - cost {TAGS[r][0]}| / max |cost| = {float((ct - co).abs().max() / co.abs().max()):.2e}"
                if with_grad:
                    line += f"; max |grad T - grad {TAGS[r][0]}| / max |grad| = {float((gt - go).abs().max() / go.abs().max()):.2e}"
                lines.append(line)
            record[f"{row}_{B}"] = {"tile64_ms": tt, **{f"{r}_ms": med[TAGS[r]] for r in others}}
            del ys
            torch.cuda.empty_cache()
    lines.append("not measured: hardware counters (LDS bank conflicts, LDS-DMA overlap, MFMA busy); one column block per wave "
                 "(only the two-block instances were built); other window sizes than the default")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "soft_cost_tile64", **record}))


if __name__ == "__main__":
    main()
