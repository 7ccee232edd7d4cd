"""The fused fp64 mapper (fuse_mapper64=True: nn.Linear inside the fp64 matrix-core forward, the MAPPED instances of
rayen_mfma_f64.hip) against the two-op route (a library GEMM that writes v, then the same forward reading it back), fp64,
through the module.

  c3_64     config 3 + Linear(64, 64),  B = 262 144    inference; forward + backward
  c5_64     config 5 + Linear(64, 30),  B = 262 144    inference; forward + backward   (the reference harness's own layer)
  c5_64s    config 5 + Linear(64, 30),  B = 16 384     inference; forward + backward
  c2_64     config 2 + Linear(64, 16),  B = 4 096      inference
  c3_256    config 3 + Linear(256, 64), B = 262 144    inference

The protocol of scripts/bench_wide_fused64.py: HIP events around timing windows of calls; a route is warm when two
consecutive timing windows agree within 2 %; every call takes the next of the rotating inputs (together larger than the
256 MiB Infinity Cache); both routes run in this process, alternating timing window by timing window.  The two-op route is
code this feature does not touch: it is the "before".  Inference is the module's call under no_grad with check_nan off (the
flag read is a host synchronisation); forward + backward is y = layer(x), y.backward(G) with x and the mapper's parameters
requiring gradients.  Reported per route: ms per call, and for the inference rows the useful TFLOP/s of the launch
(2 B n in_dim for the mapper + 2 B n rows of W_ext for the walk) against the 78.6 TFLOP/s fp64 matrix peak.  Lines go to
stdout and are appended to --out.
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

from bench_wide_fused import warm, window                       # noqa: E402
from rayen_amd import _lib, workloads                           # noqa: E402
from rayen_amd.constraint_module import ConstraintModule        # noqa: E402

PEAK = 78.6e12             # fp64 matrix cores, flop / s
DEV = "cuda:0"
SHAPES = {                 # name: (config, in_dim, B, also forward + backward)
    "c3_64": ("c3", 64, 262144, True),
    "c5_64": ("c5", 64, 262144, True),
    "c5_64s": ("c5", 64, 16384, True),
    "c2_64": ("c2", 64, 4096, False),
    "c3_256": ("c3", 256, 262144, False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--calls", type=int, default=10, help="calls per timing window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "mapper64.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mapper64.py measures on an MI355X; no HIP device here")
    os.environ["RAYEN_STRICT_HIP"] = "1"
    torch.set_default_dtype(torch.float64)
    lines, record = [f"calls per timing window {args.calls}, timing windows {args.windows}"], {}
    layers = {}
    for name in args.shapes.split(","):
        config, d, B, with_bwd = SHAPES[name]
        t0 = time.time()
        if (config, d) not in layers:
            cs = workloads.build_constraints(workloads.make_raw(config, seed=0))
            torch.manual_seed(0)
            layers[(config, d)] = (cs, ConstraintModule(cs, input_dim=d, create_map=True, fuse_mapper64=True).to(DEV))
        cs, layer = layers[(config, d)]
        layer.check_nan = False
        dp = layer.device_pack(torch.device(DEV))[0]
        n, k = cs.n, cs.k
        rows = dp.consts.W.shape[0] + (0 if dp.consts.out_identity else k)
        count = max(2, -(-(600 << 20) // (B * d * 8)))
        xs = [torch.empty(B, d, device=DEV).uniform_(-2, 2) for _ in range(count)]
        G = torch.empty(B, k, 1, device=DEV).uniform_(-1, 1)
        lines.append(f"{name}: config {config[1:]} (n = {n}, k = {k}, {rows} rows of W_ext) + Linear({d}, {n}), B = {B}, {count} "
                     f"rotating inputs of {B * d * 8 / 2 ** 20:.1f} MiB; v is {B * n * 8 / 1e6:.1f} MB (setup {time.time() - t0:.1f} s)")
        assert dp.mapper_mode64(d) == 1, name
        turn = [0]

        def infer(fuse):
            def run():
                layer.fuse_mapper64 = fuse
                i = turn[0] % len(xs)
                turn[0] += 1
                with torch.no_grad():
                    return layer(xs[i])
            return run

        def train(fuse):
            def run():
                layer.fuse_mapper64 = fuse
                i = turn[0] % len(xs)
                turn[0] += 1
                x = xs[i].requires_grad_(True)
                x.grad = None
                layer.mapper.weight.grad = None
                layer.mapper.bias.grad = None
                layer(x).backward(G)
            return run

        y_f, y_t = infer(True)(), None
        assert _lib.load().rayen_last_forward_kernel() == _lib.KERNEL_MFMA
        turn[0] -= 1
        y_t = infer(False)()
        lines.append(f"    largest difference of y on one input, fused against two-op: {float((y_f - y_t).abs().max()):.3e}")
        del y_f, y_t
        modes = [("inference", infer)] + ([("forward + backward", train)] if with_bwd else [])
        for mode, make in modes:
            paths = [("two-op", make(False)), ("fused", make(True))]
            for label, run in paths:
                lines.append(f"    {mode}, {label}: warm after {warm(run, args.calls)} timing windows of {args.calls} calls")
            times = {label: [] for label, _ in paths}
            for _ in range(args.windows):
                for label, run in paths:
                    times[label].append(window(run, args.calls))
            flops = 2.0 * B * n * (d + rows)
            for label, _ in paths:
                t = np.array(times[label])
                ms = float(np.median(t))
                useful = ""
                if mode == "inference":
                    useful = (f"   useful {flops / (ms * 1e-3) / 1e12:.2f} TFLOP/s = {flops / (ms * 1e-3) / PEAK:.1%} of the fp64 "
                              "matrix peak" + (" (both launches)" if label == "two-op" else ""))
                lines.append(f"    {mode}, {label}: median {ms:.4f} ms  min {t.min():.4f}  max {t.max():.4f}{useful}")
                record[f"{name}_{mode.replace(' + ', '_').replace(' ', '_')}_{label}_ms"] = ms
            key = f"{name}_{mode.replace(' + ', '_').replace(' ', '_')}"
            tt, tf = record[key + "_two-op_ms"], record[key + "_fused_ms"]
            lines.append(f"    {mode}: two-op / fused = {tt / tf:.2f} x ({'fused faster' if tf < tt else 'fused NOT faster'})")
        for x in xs:
            x.requires_grad_(False)
        del xs, G
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "mapper64", **record}))


if __name__ == "__main__":
    main()
