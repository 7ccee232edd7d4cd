"""The streamed Bar kernels (rayen_bar_stream.hip) against what served their layers before.

  --part rows     12-D box fp32 and 11-D box fp64 (beyond the resident envelope), B = 262 144 and 4 096, forward and
                  forward + backward:  S  bar_kernel='stream'  against  T  the torch formula on the device (_bar_reference)
                  10-D box fp32, B = 262 144:  S against R  the resident kernel (a record: 'auto' takes R there)
  --part window   the 12-D box fp32, B = 262 144, at windows of 20 KiB, 40 KiB and the largest (81 664 bytes)
  --part grid     six window sizes on the 12-D box's shape (fp32) and the 11-D box's (fp64), straight through ops
  --part rtable   every K and precision on 4 096 generators (K = 16: the 12-D box's shape), straight through
                  ops.bar_forward_raw / bar_backward_raw
grid and rtable run at the R (rows a lane group carries at once) of the process: RAYEN_BAR_STREAM_ROWS = 1, 2 or 4 in the
environment, which the library reads once; run them once per R.  window and grid pass windows beyond the default, which
the library accepts only with RAYEN_BAR_STREAM_MEASURE=1 in the environment.

The protocol of scripts/bench_soft_cost_stream.py: HIP events around timing windows of calls; a path is warm when two
consecutive timing windows agree within 2 %; every call takes the next of the rotating inputs (together larger than the
256 MiB Infinity Cache); the paths of a row run in this process, alternating timing window by timing window.  Lines go to
stdout and are appended to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rayen_amd import ops, workloads                            # noqa: E402
from rayen_amd.constraint_module import ConstraintModule        # noqa: E402

HBM_RATE = 6.3e12          # bytes / s: the achievable rate the project prices against
DEV = "cuda:0"
LDS, YP_BYTES = 160 * 1024, 512
MAX_WINDOW = (LDS - YP_BYTES) // 2 // 16 * 16


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


def measure(paths, windows, lines):
    """paths: [(label, fn, calls)]; alternating timing windows; returns label -> median ms."""
    for label, fn, calls in paths:
        lines.append(f"    {label}: warm after {warm(fn, calls)} timing windows of {calls} calls")
    times = {}
    for _ in range(windows):
        for label, fn, calls in paths:
            times.setdefault(label, []).append(window(fn, calls))
    out = {}
    for label, _, _ in paths:
        t = np.array(times[label])
        out[label] = float(np.median(t))
        lines.append(f"    {label}: median {np.median(t):.4f} ms  min {t.min():.4f}  max {t.max():.4f}")
    return out


def box(d, **kw):
    raw = workloads._empty(d)
    raw["A1"], raw["b1"] = np.r_[np.eye(d), -np.eye(d)], np.ones((2 * d, 1))
    return ConstraintModule(workloads.build_constraints(raw), method="Bar", create_map=False, **kw).to(DEV)


def lanes(m):
    L = 1
    while L < (m + 3) // 4 and L < 16:
        L *= 2
    return L


def rows_table(K, f64):          # rayen_bar_stream_layout.h: bar_stream_rows
    return int(os.environ.get("RAYEN_BAR_STREAM_ROWS", "0")) or 1


def rotating(B, m, k, dtype, budget=600 << 20):
    n = max(2, -(-budget // (B * m * torch.empty(0, dtype=dtype).element_size())))
    qs = [torch.empty(B, m, 1, dtype=dtype, device=DEV).uniform_(-5, 5) for _ in range(n)]
    gys = [torch.randn(B, k, 1, dtype=dtype, device=DEV) for _ in range(n)]
    return qs, gys


def module_paths(modules, qs, gys, backward, calls):
    """modules: [(label, callable q -> y)]"""
    turn = [0]

    def step(f):
        def run():
            i = turn[0] % len(qs)
            turn[0] += 1
            if backward:
                q = qs[i]
                q.grad = None
                f(q).backward(gys[i])
            else:
                with torch.no_grad():
                    f(qs[i])
        return run
    return [(label, step(f), c) for (label, f), c in zip(modules, calls)]


def traffic(lines, label, ms, B, m, K, elem, backward):
    """Bytes of q (+ the backward's q and grad_q) per second, and what the workgroups re-read of the image from L2: one
    sweep of the image per pass of the forward, two per pass of the backward (vertex windows, then all windows)."""
    moved = B * m * elem * (3 if backward else 1)
    rpp = (512 // lanes(m)) * rows_table(K, elem == 8)
    image = ((m + 3) // 4 * 4) * K * elem
    sweeps = 3 if backward else 1
    lines.append(f"    {label}: q{' + q + grad_q' if backward else ''} = {moved / 2 ** 30:.2f} GiB -> {moved / (ms * 1e-3) / 1e12:.2f} TB/s = "
                 f"{moved / (ms * 1e-3) / HBM_RATE:.1%} of 6.3 TB/s; image re-read from L2: B / {rpp} rows per pass x "
                 f"{image / 1024:.0f} KiB x {sweeps} sweep{'s' if sweeps > 1 else ''} = {-(-B // rpp) * image * sweeps / 1e9:.2f} GB")


def part_rows(args, lines, record):
    os.environ.pop("RAYEN_STRICT_HIP", None)
    for d, dtype, other in ((12, torch.float32, "torch"), (11, torch.float64, "torch"), (10, torch.float32, "resident")):
        layer = box(d, bar_kernel="stream", bar_window_bytes=args.window_bytes)
        base = box(d) if other == "resident" else None
        bp, _ = layer.bar_pack(torch.device(DEV))
        assert bp.resident_served(dtype) == (other == "resident")
        m, k, K, elem = 2 ** d, d, 16, 4 if dtype == torch.float32 else 8
        for B in ((262144, 4096) if other == "torch" else (262144,)):
            qs, gys = rotating(B, m, k, dtype)
            for backward in (False, True):
                for q in qs:
                    q.requires_grad_(backward)
                tag = "T torch formula" if other == "torch" else "R resident"
                slow = max(args.calls // 5, 2) if (other == "torch" and B > 4096) else args.calls
                f_other = layer._bar_reference if other == "torch" else base
                name = f"{d}-D box {str(dtype).split('.')[-1]} B={B} {'forward + backward' if backward else 'forward'}"
                lines.append(f"  {name}: {m} vertices, K = {K}, image {m * K * elem // 1024} KiB, {len(qs)} rotating inputs of "
                             f"{B * m * elem / 2 ** 20:.0f} MiB")
                t = measure(module_paths([("S stream", layer), (tag, f_other)], qs, gys, backward, [args.calls, slow]), args.windows, lines)
                ts, to = t["S stream"], t[tag]
                lines.append(f"    S against {tag[0]}: {to / ts:.2f} x ({'S faster' if ts < to else 'S NOT faster'})")
                traffic(lines, "S", ts, B, m, K, elem, backward)
                record[f"box{d}_{B}_{'fb' if backward else 'f'}"] = {"stream_ms": ts, f"{other}_ms": to}
            del qs, gys
            torch.cuda.empty_cache()


def part_window(args, lines, record):
    """Needs RAYEN_BAR_STREAM_MEASURE=1 in the environment: 40 and 80 KiB are beyond the default window."""
    layer = box(12, bar_kernel="stream")
    B, m, k = 262144, 4096, 12
    qs, gys = rotating(B, m, k, torch.float32)
    for backward in (False, True):
        for q in qs:
            q.requires_grad_(backward)

        def at(w):
            def f(q):
                layer.bar_window_bytes = w
                return layer(q)
            return f
        sizes = [20 * 1024, 40 * 1024, MAX_WINDOW]
        lines.append(f"  12-D box float32 B={B} {'forward + backward' if backward else 'forward'}: windows of {sizes} bytes "
                     f"(LDS of a workgroup: 512 + 2 windows; workgroups per CU by LDS: {[min(4, LDS // (512 + 2 * w)) for w in sizes]})")
        t = measure(module_paths([(f"window {w}", at(w)) for w in sizes], qs, gys, backward, [args.calls] * 3), args.windows, lines)
        record[f"window_{'fb' if backward else 'f'}"] = t


def part_rtable(args, lines, record):
    """One R per process: the library reads RAYEN_BAR_STREAM_ROWS once, at its first streamed call.  Run this part once per
    R (the environment set by the caller) and compare the lines; the processes run one after another on the same device."""
    R = rows_table(0, 0)
    m, B = 4096, 65536
    for dtype in (torch.float32, torch.float64):
        elem = 4 if dtype == torch.float32 else 8
        for K in (4, 8, 16, 32, 64):
            cap = 4 if (K <= 8 if elem == 8 else K <= 32) else 2 if (K <= 32 if elem == 8 else True) else 1
            if R > cap:
                lines.append(f"  {str(dtype).split('.')[-1]} K={K} R={R}: no such instance (its state does not fit the registers)")
                continue
            rng = np.random.default_rng(K)
            bp = ops.BarPack(rng.uniform(-1, 1, size=(K, m)), rng.uniform(-1, 1, size=K), m, 0, 0)
            qs, gys = rotating(B, m, K, dtype)
            qs, gys = [q[:, :, 0] for q in qs], [g[:, :, 0] for g in gys]
            turn = [0]

            def fwd():
                i = turn[0] % len(qs)
                turn[0] += 1
                return qs[i], gys[i], ops.bar_forward_raw(qs[i], bp, kernel="stream", window_bytes=args.window_bytes)

            def both():
                q, gy, (_, lse) = fwd()
                ops.bar_backward_raw(q, lse, gy, bp, kernel="stream", window_bytes=args.window_bytes)
            for label, fn in (("forward", fwd), ("forward + backward", both)):
                warm(fn, args.calls)
                t = [window(fn, args.calls) for _ in range(args.windows)]
                lines.append(f"  {str(dtype).split('.')[-1]} K={K} m={m} B={B} window {args.window_bytes or 'default'} R={R} {label}: "
                             f"median {np.median(t):.4f} ms ({min(t):.4f} .. {max(t):.4f})")
                record[f"rtable_{elem * 8}_{K}_{R}_{'fb' if label != 'forward' else 'f'}"] = float(np.median(t))
            bp.close()
            del qs, gys
            torch.cuda.empty_cache()


def part_grid(args, lines, record):
    """Window size on the 12-D box's shape (fp32) and the 11-D box's (fp64), straight through ops, at the R of this process
    (RAYEN_BAR_STREAM_ROWS; default: the shipped table).  Window and R interact through occupancy: a workgroup's LDS is
    512 + 2 windows, its registers grow with R.  Needs RAYEN_BAR_STREAM_MEASURE=1 for windows beyond the default."""
    B, R = 65536, rows_table(0, 0)
    for dtype, m in ((torch.float32, 4096), (torch.float64, 2048)):
        K = 16
        rng = np.random.default_rng(K)
        bp = ops.BarPack(rng.uniform(-1, 1, size=(K, m)), rng.uniform(-1, 1, size=K), m, 0, 0)
        qs, gys = rotating(B, m, K, dtype)
        qs, gys = [q[:, :, 0] for q in qs], [g[:, :, 0] for g in gys]
        turn = [0]
        for backward in (False, True):
            cells = []
            for w in (8 * 1024, 16 * 1024, 20 * 1024, 26 * 1024, 40 * 1024, MAX_WINDOW):
                def fn():
                    i = turn[0] % len(qs)
                    turn[0] += 1
                    _, lse = ops.bar_forward_raw(qs[i], bp, kernel="stream", window_bytes=w)
                    if backward:
                        ops.bar_backward_raw(qs[i], lse, gys[i], bp, kernel="stream", window_bytes=w)
                warm(fn, args.calls)
                t = float(np.median([window(fn, args.calls) for _ in range(args.windows)]))
                cells.append(f"{w}: {t:.4f}")
                record[f"grid_{str(dtype).split('.')[-1]}_{'fb' if backward else 'f'}_{w}_{R}"] = t
            lines.append(f"  {str(dtype).split('.')[-1]} K={K} m={m} B={B} R={R} {'forward + backward' if backward else 'forward'}, "
                         "median ms by window bytes: " + "  ".join(cells))
        bp.close()
        del qs, gys
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="rows", choices=["rows", "window", "rtable", "grid"])
    ap.add_argument("--calls", type=int, default=10, help="calls per timing window (the torch formula at B = 262 144: a fifth, at least 2)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-bytes", type=int, default=0, help="the streamed kernels' window in --part rows (0: the default)")
    ap.add_argument("--out", default=os.path.join("profiles", "bench", "bar_stream.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bar_stream.py measures on an MI355X; no HIP device here")
    lines, record = [f"--part {args.part} (calls per timing window {args.calls}, timing windows {args.windows})"], {}
    {"rows": part_rows, "window": part_window, "rtable": part_rtable, "grid": part_grid}[args.part](args, lines, record)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "bar_stream", "part": args.part, **record}))


if __name__ == "__main__":
    main()
