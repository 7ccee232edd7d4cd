#!/usr/bin/env python
"""Developer measurement (round 9): where a launch of the W-in-LDS forward spends the time it does not spend in its steady
state.  With a -DRAYEN_WL_CLOCK build every wave of every 16th workgroup stamps its entry, its first MFMA, the end of its first
group and its exit (s_memrealtime, 100 MHz) and reports its SIMD (HW_ID); per SIMD this prints how long it ran with 4, 3, 2, 1
and 0 of its waves alive, the time from entry to the first MFMA, and the launch time against the last wave's exit:
    RAYEN_HIP_LIBRARY=.../librayen_mfma_pair_wl_clock.so python scripts/ubench/wl_drain.py [--batches ...] [--drain 0,1]"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rayen_amd import _lib, ops, workloads  # noqa: E402
from rayen_amd.constraint_module import ConstraintModule  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="262144,1048576")
ap.add_argument("--drain", default="0,1")
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()
lib = _lib.load()
lib.rayen_pair_schedule(3)
raw = ctypes.CDLL(os.environ["RAYEN_HIP_LIBRARY"])
cs = workloads.build_constraints(workloads.make_raw("c3", seed=args.seed))
layer = ConstraintModule(cs, create_map=False).cuda()
dp, _ = layer.device_pack(torch.device("cuda", 0))
SLOTS = 10


def med(x):
    return float(np.median(x)) if len(x) else float("nan")


for B in [int(b) for b in args.batches.split(",")]:
    x = torch.empty(B, cs.n, device="cuda").uniform_(-1, 1, generator=torch.Generator(device="cuda").manual_seed(1))
    y = torch.empty(B, cs.k, device="cuda")
    for drain in [int(d) for d in args.drain.split(",")]:
        lib.rayen_pair_drain(drain)
        for _ in range(300):
            ops.project_raw(x, dp, want_active=False, want_kappa=False, out=y)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            ops.project_raw(x, dp, want_active=False, want_kappa=False, out=y)
        e1.record()
        torch.cuda.synchronize()
        assert lib.rayen_last_forward_kernel() == _lib.KERNEL_PAIR_WL
        buf = np.zeros(16 * 16 * SLOTS, dtype=np.uint64)
        assert raw.rayen_debug_wl_clock(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(buf.nbytes)) == 0
        b = buf.reshape(16, 16, SLOTS)
        b = b[(b[:, :, 7] > b[:, :, 1]).all(axis=1)]                      # (workgroups of the LAST launch that ran all their waves)
        rt = b[:, :, 1:8:2].astype(np.float64) * 0.01                     # us: entry, first MFMA, end of first group, exit
        ticks = (b[:, :, 6] - b[:, :, 0]).astype(np.float64)
        simd = ((b[:, :, 8] >> np.uint64(4)) & np.uint64(3)).astype(np.int64)
        groups = b[:, :, 9].astype(np.int64)
        start, end = rt[:, :, 0].min(), rt[:, :, 3].max()
        alive = {k: [] for k in (4, 3, 2, 1, 0)}
        idle_cu = []
        per_simd_waves = []
        for w in range(b.shape[0]):
            wg_end = rt[w, :, 3].max()
            for s in range(4):
                on = simd[w] == s
                per_simd_waves.append(int(on.sum()))
                if on.sum() != 4:
                    continue
                ex = np.sort(rt[w, on, 3])
                t0 = rt[w, on, 0].min()
                alive[4].append(ex[0] - t0)
                alive[3].append(ex[1] - ex[0])
                alive[2].append(ex[2] - ex[1])
                alive[1].append(ex[3] - ex[2])
                alive[0].append(end - ex[3])
                idle_cu.append(wg_end - ex[3])
        head = (rt[:, :, 1] - rt[:, :, 0]).ravel()
        first = (rt[:, :, 2] - rt[:, :, 1]).ravel()
        life = (rt[:, :, 3] - rt[:, :, 0]).ravel()
        ghz = ticks.ravel() / (life * 1e-6) / 1e9
        print(f"c3 seed {args.seed} B={B} drain={drain}: {e0.elapsed_time(e1) * 10:.2f} us per launch (events around 100 calls); "
              f"{b.shape[0]} workgroups probed, first entry to last exit {end - start:.2f} us, entries spread over "
              f"{rt[:, :, 0].max() - start:.2f} us; shader clock {med(ghz):.3f} GHz", flush=True)
        print(f"   waves per SIMD seen: {sorted(set(per_simd_waves))}; groups per wave: min {groups.min()} median {med(groups.ravel()):.0f} "
              f"max {groups.max()}")
        print(f"   entry -> first MFMA   median {med(head):.2f} us  max {head.max():.2f}      first MFMA -> end of first group   median "
              f"{med(first):.2f}  min {first.min():.2f}  max {first.max():.2f}      wave life  median {med(life):.2f}  min {life.min():.2f}  max {life.max():.2f}")
        print("   per SIMD, us with k of its four waves alive (median | mean over the probed SIMDs):")
        for k in (4, 3, 2, 1, 0):
            what = "  (to the launch's last exit)" if k == 0 else ""
            print(f"      {k} alive   {med(alive[k]):7.2f} | {float(np.mean(alive[k])) if alive[k] else float('nan'):7.2f}{what}")
        print(f"      0 alive, to the last exit of the SIMD's own workgroup   {med(idle_cu):7.2f} | {float(np.mean(idle_cu)) if idle_cu else float('nan'):7.2f}")
