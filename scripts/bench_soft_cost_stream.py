"""The streamed soft cost (rayen_cost_stream.hip) against what served its sets before, loss + gradient per call:

  (a) config 5 (k = 45, ~1.1 k corridor rows, 72 quadratics, 15 equalities), fp32, B = 262 144 and 16 384:
      S  SoftCost(cs, kernel='stream')        against      M  the mirror (soft_cost.py in torch ops) on the device
  (b) config 3 (k = 64, 128 linear rows, 4 quadratics, 2 cones), fp64, B = 262 144:    S against M
  (c) config 3, fp32, B = 262 144:    S against R  SoftCost(cs) on the resident kernel (a record: 'auto' prefers R)

The protocol of scripts/bench_soft_cost.py: HIP events around timing windows of calls (not to be confused with the windows
the image is cut into); a path is warm when two consecutive timing windows agree within 2 %; every call takes the next of ROTATE input buffers; the two paths of a row run in this process, alternating
timing window by timing window.  A call is ``cost = module(y); cost.sum().backward()``.  Lines go to stdout and to
profiles/bench/soft_cost_stream.txt (--out).
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

from rayen_amd import workloads                           # noqa: E402
from rayen_amd.soft_cost import SoftCost                  # noqa: E402

PEAK_F32_MFMA = 157.3e12          # MI355X, v_mfma_f32_32x32x2_f32
TILE_BYTES32 = 4 * (2048 + 32 + 8)
ROWS = {"a": ("c5", torch.float32, (262144, 16384), "mirror"), "b": ("c3", torch.float64, (262144,), "mirror"),
        "c": ("c3", torch.float32, (262144,), "resident")}


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


def tiles32(a):
    """(tiles of the first product, tiles of the coefficient product) of the fp32 image: the quadratics reuse P y."""
    lin = -(-a["b1"].size // 32) + -(-a["b2"].size // 32)
    cones = sum(2 if r > 32 else 1 for r in a["soc_rows"])
    return lin + 2 * a["r"].size + cones, lin + cones


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="a,b,c")
    ap.add_argument("--calls", type=int, default=10, help="calls per timing window (the mirror: a fifth of it, at least 2)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=6)
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "soft_cost_stream.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_soft_cost_stream.py measures on an MI355X; no HIP device here")
    os.environ.pop("RAYEN_STRICT_HIP", None)          # (the mirror is one of the paths)
    lines, record, sets = [], {}, {}
    for row in args.rows.split(","):
        config, dtype, batches, other = ROWS[row]
        if config not in sets:
            sets[config] = workloads.build_constraints(workloads.make_raw(config, seed=0))
        cs = sets[config]
        k = cs.k
        stream = SoftCost(cs, kernel="stream").cuda()
        base = SoftCost(cs).cuda()
        a = stream.arrays
        for B in batches:
            rng = np.random.default_rng(0)
            y0 = torch.from_numpy(np.asarray(cs.y0, dtype=np.float64).reshape(1, k))
            span = 1.0 + float(y0.abs().max())
            scale = torch.from_numpy(rng.choice([0.02, 0.3, 1.5], size=(B, 1)))
            ys = [(y0 + span * (torch.rand((B, k), dtype=torch.float64, generator=torch.Generator().manual_seed(i)) * 2 - 1) * scale)
                  .to(dtype).cuda().requires_grad_(True) for i in range(args.rotate)]
            turn = [0]

            def step(module):
                def run():
                    y = ys[turn[0] % len(ys)]
                    turn[0] += 1
                    y.grad = None
                    module(y).sum().backward()
                return run

            pack, _ = stream.cost_pack(ys[0].device)
            assert pack.stream_served(dtype) and pack.served(dtype) == (other == "resident")
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)          # (the default module says once that it runs the mirror)
                base(ys[0].detach())
            assert bool(base._unsupported) == (other == "mirror")
            tag = {"mirror": "M mirror", "resident": "R resident"}[other]
            paths = [("S stream", step(stream), args.calls), (tag, step(base), args.calls if other == "resident" else max(args.calls // 5, 2))]
            name = f"({row}) {config} {str(dtype).split('.')[-1]} B={B}"
            lines.append(f"{name}: k={k}, rows {a['b1'].size} + {a['r'].size} quadratics + {a['soc_rows'].size} cones + {a['b2'].size} equalities; "
                         f"{args.windows} timing windows, {args.rotate} rotating inputs of {B * k * ys[0].element_size() / 2 ** 20:.0f} MiB")
            times = {}
            for label, fn, calls in paths:
                lines.append(f"  {label}: warm after {warm(fn, calls)} timing windows of {calls} calls")
            for _ in range(args.windows):
                for label, fn, calls in paths:
                    times.setdefault(label, []).append(window(fn, calls))
            for label, _, _ in paths:
                t = np.array(times[label])
                lines.append(f"  {label}: median {np.median(t):.4f} ms  min {t.min():.4f}  max {t.max():.4f}")
            ts, to = float(np.median(times["S stream"])), float(np.median(times[tag]))
            verdict = "S faster" if ts < to else "S NOT faster"
            lines.append(f"  S against {tag[0]}: {to / ts:.2f} x ({verdict})")
            if dtype == torch.float32:
                first, second = tiles32(a)
                flops = 2.0 * B * 32 * 64 * (first + second)          # what the matrix cores execute: whole tiles of 32 x 64
                useful = 2.0 * B * k * ((a["b1"].size + a["b2"].size + int(a["soc_rows"].sum())) * 2 + a["r"].size * k)
                image = first * TILE_BYTES32 + 256 * (a["r"].size + a["soc_rows"].size)
                lines.append(f"  S: {useful / 1e9:.1f} useful GFLOP ({flops / 1e9:.1f} executed in whole tiles) -> {useful / (ts * 1e-3) / 1e12:.1f} "
                             f"useful TFLOP/s = {useful / (ts * 1e-3) / PEAK_F32_MFMA:.1%} of the fp32 MFMA peak (157.3 TF), the module's "
                             f"host work and backward multiply included; image re-read per 128 samples: {image / 1024:.0f} KiB "
                             f"({image * -(-B // 128) / 1e9:.2f} GB per call from L2)")
            # the same numbers from both paths
            y = ys[0]
            y.grad = None
            cs_ = stream(y)
            cs_.sum().backward()
            gs, cs_ = y.grad.clone(), cs_.detach()
            y.grad = None
            cb = base(y)
            cb.sum().backward()
            cb = cb.detach()
            lines.append(f"  agreement: max |cost S - cost {tag[0]}| / max |cost| = {float((cs_ - cb).abs().max() / cb.abs().max()):.2e}; "
                         f"max |grad S - grad {tag[0]}| / max |grad| = {float((gs - y.grad).abs().max() / y.grad.abs().max()):.2e}")
            record[f"{row}_{B}"] = {"stream_ms": ts, f"{other}_ms": to}
            del ys
            torch.cuda.empty_cache()
    lines.append("not measured: hardware counters (LDS-DMA overlap, L2 hit rate); a single-buffered variant of the kernel (only the "
                 "double-buffered one was built)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "soft_cost_stream", **record}))


if __name__ == "__main__":
    main()
