"""Euclidean projection (``ProjectionModule``), fp32: the tile kernel (rayen_amd/csrc/rayen_proj_tile.hip, 32 samples per
workgroup on the matrix cores) against what served the same call before it.

  (a) config 3 (n = 64, 522 cone rows, 6 cones), B = 262 144, eps 1e-6, max_iters 512, forward and forward + backward:
        W  kernel='wave': rayen_proj.hip, one wave per sample, the image in LDS
        T  kernel='tile'
  (b) config 5 (``workloads.make_raw("c5")``: n = 30, 1 410 cone rows, 72 cones; outside the wave kernel's envelope),
      B = 16 384, both paths stopped at the same small ``--max-iters-c5``:
        M  projection.mirror_forward / mirror_backward on the device: the same iteration in torch ops
        T  kernel='tile'

HIP events around windows of calls; a path is warm when two consecutive windows agree within 2 %.  Both paths of a
comparison run in this process, alternating windows.  The fraction of the fp32 MFMA peak (157.3 TFLOP/s) counts the USEFUL
arithmetic of the iterations the rows took: sum over rows of iters x 2 (2 m n + n^2) flop, over the forward's time -- not
the padded products the kernel executes.  Lines go to stdout and to profiles/bench/proj_tile.txt (--out).  No ratio is
expected in advance; no hardware counters are collected here.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rayen_amd import ops, projection, workloads                # noqa: E402

PEAK_FP32_MFMA = 157.3e12


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


def compare(lines, result, key, what, paths, args):
    times = {}
    for label, fn in paths:
        lines.append(f"  {what}, {label}: warm after {warm(fn, args.calls, args.warm_limit)} windows")
    for _ in range(args.windows):                      # alternate the paths window by window
        for label, fn in paths:
            times.setdefault(label, []).append(window(fn, args.calls))
    for label, _ in paths:
        t = np.array(times[label])
        lines.append(f"  {what}, {label}: median {np.median(t):.3f} ms  min {t.min():.3f}  max {t.max():.3f}")
    (la, _), (lb, _) = paths
    ta, tb = float(np.median(times[la])), float(np.median(times[lb]))
    lines.append(f"  {what}, T against {la[0]}: {ta / tb:.2f} x ({'T faster' if tb < ta else 'T NOT faster: the tile kernel loses here'})")
    result[f"{key} {what}"] = {"before_ms": ta, "tile_ms": tb}
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--warm-limit", type=int, default=4)
    ap.add_argument("--max-iters", type=int, default=512)
    ap.add_argument("--max-iters-c5", type=int, default=64)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--batch-c3", type=int, default=262144)
    ap.add_argument("--batch-c5", type=int, default=16384)
    ap.add_argument("--only", choices=("c3", "c5"), default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "proj_tile.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_proj_tile.py measures on an MI355X; no HIP device here")

    lines, result = [], {"bench": "proj_tile"}
    # name -> (amp of the inputs, rho (None: build_program probes), batch, max_iters, the path before the tile kernel)
    plan = {"c3": (0.02, 30.0, args.batch_c3, args.max_iters, "wave"), "c5": (0.1, None, args.batch_c5, args.max_iters_c5, "mirror")}
    for name, (amp, rho, B, max_iters, before) in plan.items():
        if args.only and name != args.only:
            continue
        cs = workloads.build_constraints(workloads.make_raw(name))
        layers = {k: projection.ProjectionModule(cs, create_map=False, rho=rho, max_iters=max_iters, eps=args.eps,
                                                 kernel=k).cuda() for k in ("wave", "tile")}
        prog = layers["tile"].program
        def inputs(amp):
            rng = np.random.default_rng(0)
            q = cs.z0.reshape(1, -1) + amp * rng.uniform(0.0, 1.5, (B, 1)) * rng.standard_normal((B, cs.n))
            return torch.from_numpy(q).float().cuda(), rng

        # the amplitude of the inputs: the table's, tripled until at most half of the leading 1 024 rows are inside the set
        # (rows inside take no iteration and measure nothing)
        while True:
            q, rng = inputs(amp)
            with torch.no_grad():
                _, probe = layers["tile"].project(q[:1024], max_iters=1)
            if float((probe == 0).float().mean()) <= 0.5 or amp > 100.0:
                break
            amp *= 3.0
        g = torch.from_numpy(rng.standard_normal((B, cs.n))).float().cuda()
        c = layers["tile"].constants(torch.float32, q.device)

        def mirror_fwd():
            return projection.mirror_forward(c, q, max_iters, args.eps)

        def mirror_both():
            z, iters, vstar = mirror_fwd()
            return projection.mirror_backward(c, g, vstar, iters, max_iters, args.eps)

        def kernel_fwd(kind):
            def run():
                with torch.no_grad():
                    return layers[kind].project(q)
            return run

        def kernel_both(kind):
            def run():
                qg = q.detach().requires_grad_(True)
                z, _ = layers[kind].project(qg)
                z.backward(g)
                return qg.grad
            return run

        pack, _ = layers["tile"].proj_pack(q.device)
        assert ops.proj_tile_served(pack)
        lines.append(f"projection, config {name[1:]}: n={prog.n}, m={prog.m}, {len(prog.soc_rows)} cones, B={B}, fp32, "
                     f"rho={prog.rho:g}, amp={amp:g}, max_iters={max_iters}, eps={args.eps:g}; {args.windows} windows of {args.calls} calls; "
                     f"wave kernel serves it: {ops.proj_wave_served(pack, torch.float32)}")
        zt, it = kernel_fwd("tile")()
        if before == "wave":
            zb, ib = kernel_fwd("wave")()
            gb, gt = kernel_both("wave")(), kernel_both("tile")()
            paths_f = [("W wave kernel", kernel_fwd("wave")), ("T tile kernel", kernel_fwd("tile"))]
            paths_b = [("W wave kernel", kernel_both("wave")), ("T tile kernel", kernel_both("tile"))]
        else:
            zb, ib, _ = mirror_fwd()
            gb, gt = mirror_both(), kernel_both("tile")()
            paths_f = [("M mirror", mirror_fwd), ("T tile kernel", kernel_fwd("tile"))]
            paths_b = [("M mirror", mirror_both), ("T tile kernel", kernel_both("tile"))]
        assert not layers["tile"]._unsupported and not layers["wave"]._unsupported
        lines.append(f"  iterations per row: T mean {float(it.float().mean()):.1f} max {int(it.max())}; {before} mean "
                     f"{float(ib.float().mean()):.1f} max {int(ib.max())}; {float((it == 0).float().mean()):.0%} of the rows inside, "
                     f"{float((it == max_iters).float().mean()):.0%} at the limit")
        lines.append(f"  agreement: max |z - z T| / (1 + max |z|) = {float((zb - zt).abs().max() / (1 + zb.abs().max())):.2e}; "
                     f"max |grad - grad T| / (1 + max |grad|) = {float((gb - gt).abs().max() / (1 + gb.abs().max())):.2e}")
        # per row: the maximum above is over every row, kink rows included (a row whose v* has an entry within rounding of
        # a cone's boundary takes another piece of the projection's derivative on the two paths)
        rg = ((gb - gt).abs().amax(dim=1) / (1 + gb.abs().amax(dim=1))).double().cpu().numpy()
        lines.append(f"  gradient agreement per row, max |grad - grad T| / (1 + max |grad|) of the row: median {np.median(rg):.2e}, "
                     f"99 % of the rows within {np.quantile(rg, 0.99):.2e}, 99.9 % within {np.quantile(rg, 0.999):.2e}; "
                     f"{int((rg > 1e-3).sum())} of {B} rows beyond 1e-3")
        tb, tt = compare(lines, result, name, "forward", paths_f, args)
        flop = float(it.double().sum()) * 2.0 * (2.0 * prog.m * prog.n + prog.n * prog.n)
        lines.append(f"  forward, useful arithmetic {flop / 1e12:.3f} TFLOP: T {flop / (tt * 1e-3) / 1e12:.2f} TFLOP/s = "
                     f"{flop / (tt * 1e-3) / PEAK_FP32_MFMA:.1%} of the fp32 MFMA peak; before {flop / (tb * 1e-3) / 1e12:.2f} TFLOP/s = "
                     f"{flop / (tb * 1e-3) / PEAK_FP32_MFMA:.1%}")
        compare(lines, result, name, "forward + backward", paths_b, args)
        print("\n".join(lines[-16:]), flush=True)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
