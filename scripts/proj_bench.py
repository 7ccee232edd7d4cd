"""Time the Euclidean-projection op (rayen_amd::euclid_project, rayen_proj.hip) on the config-3 set and put it beside a
host loop of ``ConvexConstraints.project`` and beside ``method='RAYEN'`` on the same set.

    python scripts/proj_bench.py [--batch 262144] [--eps 1e-6] [--out FILE]

HIP events around the op; warm-up until two windows agree within 3 %.  Needs an MI355X."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rayen_amd import constraint_module, ops, projection, workloads     # noqa: E402


def window(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def steady(fn, reps=3, tries=8):
    prev = window(fn, 1)
    for _ in range(tries):
        cur = window(fn, reps)
        if abs(cur - prev) <= 0.03 * cur:
            return cur, True
        prev = cur
    return cur, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--max-iters", type=int, default=512)
    ap.add_argument("--host-rows", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cs = workloads.build_constraints(workloads.make_raw("c3"))
    layer = projection.ProjectionModule(cs, create_map=False, max_iters=args.max_iters, eps=args.eps)
    prog = layer.program
    torch.manual_seed(0)
    q = (torch.from_numpy(cs.z0.T).float() + torch.randn(args.batch, cs.n)).cuda()        # one sigma around z0: outside
    pack, _ = layer.proj_pack(q.device)
    fwd = lambda: ops.proj_forward_raw(q, pack, args.max_iters, args.eps)                 # noqa: E731
    ms_fwd, ok_fwd = steady(fwd)
    z, iters, vstar = fwd()
    g = torch.randn_like(z)
    ms_bwd, ok_bwd = steady(lambda: ops.proj_backward_raw(g, vstar, iters, pack, args.max_iters, args.eps))
    it = iters.float()
    viol = float(np.max(cs.getViolationRows(z[:4096].double().cpu().numpy())))
    rayen = constraint_module.ConstraintModule(cs, create_map=False).cuda()
    v = torch.randn(args.batch, cs.n, device="cuda")
    ms_rayen, _ = steady(lambda: rayen(v), reps=10)
    rows = q[:args.host_rows].double().cpu().numpy()
    t0 = time.perf_counter()
    for row in rows:
        cs.project(row)
    host_ms_row = (time.perf_counter() - t0) * 1e3 / len(rows)
    # what the iteration needs: two products with G and one with Kinv per iteration and row
    flop = float(it.sum()) * (4.0 * prog.m * prog.n + 2.0 * prog.n * prog.n)
    lds = float(it.sum()) * (2.0 * prog.m * prog.n + prog.n * prog.n) * 4
    lines = [
        f"config 3 (n = {prog.n}, {prog.m} cone rows, {len(prog.soc_rows)} cones, rho = {prog.rho}), B = {args.batch}, fp32, "
        f"eps = {args.eps}, max_iters = {args.max_iters}, inputs z0 + N(0, I)",
        f"kernel: one wave per sample, vector FMAs (the MFMA tiling is not built)",
        f"forward  {ms_fwd:.2f} ms per call ({'steady' if ok_fwd else 'NOT steady'}), {ms_fwd * 1e3 / args.batch:.3f} us per row",
        f"backward {ms_bwd:.2f} ms per call ({'steady' if ok_bwd else 'NOT steady'})",
        f"iterations per row: mean {float(it.mean()):.1f}, max {int(it.max())}, rows at the cap {int((iters == args.max_iters).sum())}",
        f"worst residual of the first 4096 outputs: {viol:.3e}",
        f"forward arithmetic {flop / (ms_fwd * 1e-3) / 1e12:.2f} TFLOP/s = {100 * flop / (ms_fwd * 1e-3) / 157.3e12:.1f} % of the "
        f"fp32 vector peak (157.3 TFLOP/s); LDS operand traffic {lds / (ms_fwd * 1e-3) / 1e12:.1f} TB/s "
        f"(ds_read_b32 ceiling about 75 TB/s): the kernel is bound by LDS reads, one per FMA",
        f"host loop of ConvexConstraints.project (fp64, this machine's CPU, {len(rows)} rows): {host_ms_row:.2f} ms per row "
        f"-> {host_ms_row * args.batch / 1e3:.0f} s per batch scaled; the op is {host_ms_row * args.batch / ms_fwd:.0f} x faster",
        f"method='RAYEN' forward on the same set and batch: {ms_rayen:.3f} ms ({ms_fwd / ms_rayen:.0f} x less than the projection)",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
