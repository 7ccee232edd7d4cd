"""Euclidean projection (``ProjectionModule``), fp64: the fp64 tile kernel (rayen_amd/csrc/rayen_proj_tile64.hip, 16 samples
per workgroup on the fp64 matrix cores) against what served the same fp64 call before it.

  (a) config 3 (n = 64, 522 cone rows, 6 cones; its fp64 image is over the wave kernel's LDS), B = 32 768, eps 1e-9, both
      paths stopped at the same ``--max-iters-c3`` (at B = 262 144 and 256 iterations the mirror's windows did not finish
      within seven minutes):
        M  projection.mirror_forward / mirror_backward on the device: the same iteration in torch ops
        T  kernel='tile' on fp64 input
  (b) config 5 (``workloads.make_raw("c5")``: n = 30, 1 410 cone rows, 72 cones), B = 16 384, ``--max-iters-c5``: M against T
  (c) n32_full (n = 32, 183 cone rows, 4 cones), which the fp64 wave kernel serves, B = 262 144, ``--max-iters``, for the
      record:
        W  kernel='wave'
        T  kernel='tile'

HIP events around windows of calls; a path is warm when two consecutive windows agree within 2 %.  Both paths of a
comparison run in this process, alternating windows.  The fraction of the fp64 matrix peak (78.6 TFLOP/s, bench.py's
PEAK_FP64_TFLOPS) counts the USEFUL arithmetic of the iterations the rows took: sum over rows of iters x 2 (2 m n + n^2)
flop, over the forward's time -- not the padded products the kernel executes.  Lines go to stdout and to
profiles/bench/proj_tile64.txt (--out).  No ratio is expected in advance; no hardware counters are collected here.
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
from scripts.bench_proj_tile import compare                     # noqa: E402  (windows, warming, alternation: the fp32 table's)

PEAK_FP64_MFMA = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--warm-limit", type=int, default=4)
    ap.add_argument("--max-iters", type=int, default=256)
    ap.add_argument("--max-iters-c3", type=int, default=128)
    ap.add_argument("--max-iters-c5", type=int, default=64)
    ap.add_argument("--eps", type=float, default=1e-9)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--batch-c3", type=int, default=32768)
    ap.add_argument("--batch-c5", type=int, default=16384)
    ap.add_argument("--only", choices=("c3", "c5", "n32_full"), default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "proj_tile64.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_proj_tile64.py measures on an MI355X; no HIP device here")

    lines, result = [], {"bench": "proj_tile64"}
    # name -> (the raw set, amp of the inputs, rho (None: build_program probes), batch, max_iters, the path before)
    plan = {"c3": (lambda: workloads.make_raw("c3"), 0.02, 30.0, args.batch_c3, args.max_iters_c3, "mirror"),
            "c5": (lambda: workloads.make_raw("c5"), 0.1, None, args.batch_c5, args.max_iters_c5, "mirror"),
            "n32_full": (lambda: workloads.random_lin_quad_soc(32, 48, 3, 1, seed=4), 0.1, 30.0, args.batch, args.max_iters, "wave")}
    for name, (raw, amp, rho, B, max_iters, before) in plan.items():
        if args.only and name != args.only:
            continue
        cs = workloads.build_constraints(raw())
        layers = {k: projection.ProjectionModule(cs, create_map=False, rho=rho, max_iters=max_iters, eps=args.eps,
                                                 kernel=k).double().cuda() for k in ("wave", "tile")}
        prog = layers["tile"].program

        def inputs(amp):
            rng = np.random.default_rng(0)
            q = cs.z0.reshape(1, -1) + amp * rng.uniform(0.0, 1.5, (B, 1)) * rng.standard_normal((B, cs.n))
            return torch.from_numpy(q).cuda(), rng

        # the amplitude of the inputs: the table's, tripled until at most half of the leading 1 024 rows are inside the set
        # (rows inside take no iteration and measure nothing)
        while True:
            q, rng = inputs(amp)
            with torch.no_grad():
                _, probe = layers["tile"].project(q[:1024], max_iters=1)
            if float((probe == 0).float().mean()) <= 0.5 or amp > 100.0:
                break
            amp *= 3.0
        g = torch.from_numpy(rng.standard_normal((B, cs.n))).cuda()
        c = layers["tile"].constants(torch.float64, q.device)

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
        assert ops.proj_tile64_served(pack)
        wave = ops.proj_wave_served(pack, torch.float64)
        assert wave == (before == "wave")
        lines.append(f"projection, {name}: n={prog.n}, m={prog.m}, {len(prog.soc_rows)} cones, B={B}, fp64, "
                     f"rho={prog.rho:g}, amp={amp:g}, max_iters={max_iters}, eps={args.eps:g}; {args.windows} windows of {args.calls} calls; "
                     f"fp64 wave kernel serves it: {wave}")
        zt, it = kernel_fwd("tile")()
        if before == "wave":
            zb, ib = kernel_fwd("wave")()
            gb, gt = kernel_both("wave")(), kernel_both("tile")()
            paths_f = [("W wave kernel", kernel_fwd("wave")), ("T tile64 kernel", kernel_fwd("tile"))]
            paths_b = [("W wave kernel", kernel_both("wave")), ("T tile64 kernel", kernel_both("tile"))]
        else:
            zb, ib, _ = mirror_fwd()
            gb, gt = mirror_both(), kernel_both("tile")()
            paths_f = [("M mirror", mirror_fwd), ("T tile64 kernel", kernel_fwd("tile"))]
            paths_b = [("M mirror", mirror_both), ("T tile64 kernel", kernel_both("tile"))]
        assert not layers["tile"]._unsupported and not layers["wave"]._unsupported
        lines.append(f"  iterations per row: T mean {float(it.float().mean()):.1f} max {int(it.max())}; {before} mean "
                     f"{float(ib.float().mean()):.1f} max {int(ib.max())}; {float((it == 0).float().mean()):.0%} of the rows inside, "
                     f"{float((it == max_iters).float().mean()):.0%} at the limit")
        rg = ((gb - gt).abs().amax(dim=1) / (1 + gb.abs().amax(dim=1))).cpu().numpy()
        lines.append(f"  agreement: max |z - z T| / (1 + max |z|) = {float((zb - zt).abs().max() / (1 + zb.abs().max())):.2e}; "
                     f"gradient per row, max |grad - grad T| / (1 + max |grad|): median {np.median(rg):.2e}, 99.9 % of the rows "
                     f"within {np.quantile(rg, 0.999):.2e}, max {rg.max():.2e}")
        del zb, gb, gt
        tb, tt = compare(lines, result, name, "forward", paths_f, args)
        flop = float(it.double().sum()) * 2.0 * (2.0 * prog.m * prog.n + prog.n * prog.n)
        lines.append(f"  forward, useful arithmetic {flop / 1e12:.3f} TFLOP: T {flop / (tt * 1e-3) / 1e12:.2f} TFLOP/s = "
                     f"{flop / (tt * 1e-3) / PEAK_FP64_MFMA:.1%} of the fp64 matrix peak; before {flop / (tb * 1e-3) / 1e12:.2f} TFLOP/s = "
                     f"{flop / (tb * 1e-3) / PEAK_FP64_MFMA:.1%}")
        compare(lines, result, name, "forward + backward", paths_b, args)
        print("\n".join(lines[-14:]), flush=True)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
