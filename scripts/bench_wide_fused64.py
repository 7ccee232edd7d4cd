"""The fp64 fused wide forward (wide_kernel='fused64', rayen_wide_fused64.hip) against the products route (a library GEMM
and rayen_wide.hip over its products), fp64, the forward as the module's inference call makes it (y alone).

  lin1000   the reference sweep's k = 1000 with m = 1000 linear rows, B = 2 000
  qp500     k = 500 with 100 dense quadratics, B = 2 000
  mixed256  k = 256, m = 512, 4 quadratics, 2 cones, B = 262 144 (the products matrix is about 4.3 GB)

The workloads and the protocol of scripts/bench_wide_fused.py: HIP events around timing windows of calls; a route is warm
when two consecutive timing windows agree within 2 %; every call takes the next of the rotating inputs (together larger
than the 256 MiB Infinity Cache); all routes run in this process, alternating timing window by timing window.  The fused
kernel runs with the plan's own tile (wide_samples = 0) and with 16 and 32 samples forced where the plan serves them.
Reported per route: ms per call, useful TFLOP/s (2 B n rows of W_ext) against the 78.6 TFLOP/s fp64 matrix peak, and the
bytes the route moves by its own design (not counters).  Lines go to stdout and are appended to --out.
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

from bench_wide_fused import SHAPES, warm, window               # noqa: E402
from rayen_amd import _lib, ops, workloads                      # noqa: E402
from rayen_amd.constraint_module import ConstraintModule        # noqa: E402

PEAK = 78.6e12             # fp64 matrix cores, flop / s
DEV = "cuda:0"


def plan_of(dp, samples):
    out = (ctypes.c_int64 * 13)()
    _lib.check(_lib.load().rayen_wide_fused64_plan(dp.handle, samples, out), "rayen_wide_fused64_plan")
    keys = ("n", "kp", "ks", "samples", "rows_w_pad", "nb_w", "rows_e_pad", "nb_e", "rows_pad", "scratch_words", "tile_bytes",
            "lds_bytes", "served")
    return dict(zip(keys, list(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--calls", type=int, default=10, help="calls per timing window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "wide_fused64.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide_fused64.py measures on an MI355X; no HIP device here")
    os.environ["RAYEN_STRICT_HIP"] = "1"
    torch.set_default_dtype(torch.float64)
    lines, record = [f"calls per timing window {args.calls}, timing windows {args.windows}"], {}
    for name in args.shapes.split(","):
        kw, B = SHAPES[name]
        t0 = time.time()
        cs = workloads.build_constraints(workloads.random_lin_quad_soc(**kw))
        layer = ConstraintModule(cs, create_map=False).to(DEV)
        dp = layer.device_pack(torch.device(DEV))[0]
        consts = dp.consts
        n, k = cs.n, cs.k
        rows = consts.W.shape[0] + (0 if consts.out_identity else k)
        count = max(2, -(-(600 << 20) // (B * n * 8)))
        xs = [torch.empty(B, n, device=DEV).uniform_(-1, 1) for _ in range(count)]
        lines.append(f"{name}: n = {n}, k = {k}, {rows} rows of W_ext in {len(consts.segments)} segments, B = {B}, {count} rotating "
                     f"inputs of {B * n * 8 / 2 ** 20:.0f} MiB (setup {time.time() - t0:.1f} s)")
        routes = [("products", dict(wide_kernel="products"), None)]
        for samples in (0, 16, 32):
            p = plan_of(dp, samples)
            if p["served"]:
                routes.append((f"fused64/{samples}", dict(wide_kernel="fused64", wide_samples=samples), p))
            else:
                lines.append(f"    fused64/{samples}: not served (LDS {p['lds_bytes']} B)")
        turn = [0]
        paths = []
        for label, kwargs, p in routes:
            def run(kwargs=kwargs):
                i = turn[0] % len(xs)
                turn[0] += 1
                return ops.project_raw(xs[i], dp, want_active=False, want_kappa=False, **kwargs)[0]
            run()
            kernel = _lib.load().rayen_last_forward_kernel()
            assert kernel == (_lib.KERNEL_PRODUCTS if p is None else _lib.KERNEL_WIDE_FUSED64), (label, kernel)
            paths.append((label, run, p))
        ref = ops.project_raw(xs[0], dp, want_active=False, want_kappa=False)[0]
        for label, _, p in paths[1:]:
            y = ops.project_raw(xs[0], dp, want_active=False, want_kappa=False, wide_kernel="fused64", wide_samples=int(label[8:]))[0]
            lines.append(f"    largest difference of y on one input, {label} against products: {float((y - ref).abs().max()):.3e}")
        del ref, y
        for label, run, _ in paths:
            lines.append(f"    {label}: warm after {warm(run, args.calls)} timing windows of {args.calls} calls")
        times = {label: [] for label, _, _ in paths}
        for _ in range(args.windows):
            for label, run, _ in paths:
                times[label].append(window(run, args.calls))
        flops = 2.0 * B * n * rows
        for label, _, p in paths:
            t = np.array(times[label])
            ms = float(np.median(t))
            lines.append(f"    {label}: median {ms:.4f} ms  min {t.min():.4f}  max {t.max():.4f}   useful "
                         f"{flops / (ms * 1e-3) / 1e12:.2f} TFLOP/s = {flops / (ms * 1e-3) / PEAK:.1%} of the fp64 matrix peak")
            if p is None:
                moved = (f"v {B * n * 8 / 1e6:.0f} MB read twice, T {B * rows * 8 / 1e6:.0f} MB written and read, y "
                         f"{B * k * 8 / 1e6:.0f} MB written, W_ext {rows * n * 8 / 1e6:.1f} MB")
            else:
                tiles, image = -(-B // p["samples"]), p["rows_pad"] * p["kp"] * 8
                moved = (f"tile of {p['samples']} samples, LDS {p['lds_bytes']} B; v {B * n * 8 / 1e6:.0f} MB read, y "
                         f"{B * k * 8 / 1e6:.0f} MB written" + ("" if consts.out_identity else " and read back and rewritten")
                         + f", W_ext {image / 1e6:.1f} MB from memory once and re-read from L2 by each of {tiles} tiles "
                         f"({tiles * image / 1e9:.1f} GB)")
            lines.append(f"        moves: {moved}")
            record[f"{name}_{label}_ms"] = ms
        tp = record[f"{name}_products_ms"]
        for label, _, p in paths[1:]:
            tf = record[f"{name}_{label}_ms"]
            lines.append(f"    {label} against products: {tp / tf:.2f} x ({'fused64 faster' if tf < tp else 'fused64 NOT faster'})")
        del xs, paths, layer, dp
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "wide_fused64", **record}))


if __name__ == "__main__":
    main()
