"""Generate the ``method='DC3'`` golden vectors ``tests/golden/dc3/dc3_*.npz`` from the REAL reference (a directory of
their own: the older test files take every ``tests/golden/*.npz`` for a RAYEN fixture).

Like ``make_golden.py`` (whose stand-in modules and helpers it imports) this runs only where the reference is mounted,
never on the GPU box; only its outputs are committed.  Per constraint set one file with

* the raw set, ``args_DC3`` (``lr`` halved from 1e-2 until the reference is finite in both precisions), ``q`` (fp32
  representable, used in both precisions) and the weights ``w`` of the scalar ``sum(w * y)``;
* the reference's DC3 buffers and index sets in both precisions;
* ``viol64[t-1]``: the fp64 violation after step ``t`` (the reference run with ``max_steps = t`` and ``eps_converge = 0``,
  then its stacked constraints evaluated on the output);
* per mode (``train``: ``max_steps_training = 10``; ``eval``: ``max_steps_testing = 64``) ``y32 / y64``, the step counts
  and ``d sum(w * y) / dq`` from the reference's autograd in both precisions.

``eps_converge`` is never hand-picked: it is the geometric mean of two consecutive recorded violations (the latest step
<= 45 whose violation is a new minimum by 2 %), so the stop is unambiguous; a case whose reference is not finite, whose
fp32 and fp64 runs stop at different steps, or which stops by ``max_steps`` with the last violation below ``2 eps`` is
dropped.

    python tests/golden/make_golden_dc3.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                                   # noqa: E402  (stand-ins + the reference on sys.path)
from make_golden import ref_module, workloads              # noqa: E402

T_TRAIN, T_EVAL, T_PICK = 10, 64, 45
BATCH = 48
BUFFERS = ("A2_DC3", "b2_DC3", "A1_DC3", "b1_DC3", "A2oi", "A2p", "A1_effective", "b1_effective", "all_P_effective",
           "all_q_effective", "all_r_effective")


def _layer(cs, args, dtype, training):
    torch.set_default_dtype(dtype)
    try:
        layer = ref_module.ConstraintModule(cs, method="DC3", create_map=False, args_DC3=dict(args))
    finally:
        torch.set_default_dtype(torch.float32)
    layer.train(training)
    return layer


def _run(cs, args, dtype, training, q32, w32=None):
    """(y [B,k], grad_q [B,n] | None) of the reference."""
    torch.set_default_dtype(dtype)
    try:
        layer = _layer(cs, args, dtype, training)
        torch.set_default_dtype(dtype)
        q = torch.tensor(q32).to(dtype).requires_grad_(w32 is not None)
        try:
            y = layer(q)
        except AssertionError:                             # (the reference's own NaN check, CM:531)
            return np.full((q32.shape[0], cs.k), np.nan), None
        grad = None
        if w32 is not None:
            (grad,) = torch.autograd.grad((torch.tensor(w32).to(dtype).unsqueeze(2) * y).sum(), q)
            grad = grad.numpy()[:, :, 0]
        return y.detach().numpy()[:, :, 0], grad
    finally:
        torch.set_default_dtype(torch.float32)


def _violation64(layer64, y):
    y = torch.tensor(y, dtype=torch.float64).unsqueeze(2)
    stacked = layer64.A1_DC3 @ y - layer64.b1_DC3
    for i in range(layer64.all_P.shape[0]):
        P, q, r = layer64.all_P[i], layer64.all_q[i], layer64.all_r[i]
        stacked = torch.cat((stacked, 0.5 * torch.transpose(y, 1, 2) @ P @ y + q.T @ y + r), dim=1)
    return float(torch.max(torch.relu(stacked)))


def _fixed_steps(args, t):
    return dict(args, eps_converge=0.0, max_steps_training=t, max_steps_testing=t)


def _case(name, raw, scale, seed):
    cs = mg._ref_cs_from_raw(raw)
    if cs.has_soc_constraints or cs.has_lmi_constraints:
        return
    gen = torch.Generator().manual_seed(seed)
    q32 = torch.empty(BATCH, cs.n, 1, dtype=torch.float32).uniform_(-scale, scale, generator=gen).numpy()
    w32 = torch.empty(BATCH, cs.k, dtype=torch.float32).uniform_(-1.0, 1.0, generator=gen).numpy()
    args = dict(lr=1e-2, momentum=0.5, eps_converge=0.0, max_steps_training=T_TRAIN, max_steps_testing=T_EVAL)
    # (a) finite in both precisions over the longest run
    while True:
        finite = all(np.isfinite(_run(cs, args, dt, False, q32)[0]).all() for dt in (torch.float32, torch.float64))
        if finite:
            break
        args["lr"] /= 2
        if args["lr"] < 1e-7:
            print(f"{name}: DROPPED (not finite at any lr)")
            return
    # trajectories with a fixed number of steps, both precisions; the fp64 violation after every step
    layer64 = _layer(cs, args, torch.float64, False)
    traj = {dt: [_run(cs, _fixed_steps(args, t), dt, False, q32)[0] for t in range(1, T_EVAL + 1)]
            for dt in (torch.float32, torch.float64)}
    viol = np.array([_violation64(layer64, y) for y in traj[torch.float64]])
    # (b) eps between two consecutive violations
    eps = None
    for t in range(min(T_PICK, T_EVAL - 1), 1, -1):
        before = viol[:t - 1].min()
        if 0.0 < viol[t - 1] < 0.98 * before:
            cand = float(np.sqrt(viol[t - 1] * before))
            if t > T_TRAIN and viol[T_TRAIN - 1] < 2 * cand:
                continue                                   # (training would stop by max_steps within 2 eps of the bar)
            eps = cand
            break
    if eps is None:
        if viol[-1] <= 0.0:
            print(f"{name}: DROPPED (no unambiguous stop: violations {viol[:5]} ... {viol[-3:]})")
            return
        eps = float(viol.min() / 4.0)                      # stops by max_steps, the last violation >= 2 eps
    args["eps_converge"] = eps
    data = {}
    for mode, training in (("train", True), ("eval", False)):
        limit = T_TRAIN if training else T_EVAL
        out = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            y, grad = _run(cs, args, dt, training, q32, w32)
            same = [t for t in range(1, limit + 1) if np.array_equal(traj[dt][t - 1], y)]
            if not same:
                print(f"{name}/{mode}: DROPPED (fp{tag} output matches no fixed-step run)")
                return
            out["y" + tag], out["gq" + tag], out["steps" + tag] = y, grad, same[0]
        if out["steps32"] != out["steps64"]:
            print(f"{name}/{mode}: DROPPED (fp32 stops at {out['steps32']}, fp64 at {out['steps64']})")
            return
        if out["steps64"] == limit and viol[limit - 1] < 2 * eps and not viol[limit - 1] < eps:
            print(f"{name}/{mode}: DROPPED (stops by max_steps with violation {viol[limit - 1]} < 2 eps)")
            return
        for key, val in out.items():
            data[f"{key}_{mode}"] = np.asarray(val)
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        layer = _layer(cs, args, dt, False)
        for buf in BUFFERS:
            data[f"buf_{buf}{tag}"] = getattr(layer, buf).numpy()
    data["partial_vars"] = np.asarray(layer64.partial_vars, dtype=np.int64)
    data["other_vars"] = np.asarray(layer64.other_vars, dtype=np.int64)
    data["neq_DC3"] = np.int64(layer64.neq_DC3)
    data["dim_after_map"] = np.int64(layer64.dim_after_map)
    data["args"] = np.array([args["lr"], args["momentum"], args["eps_converge"], T_TRAIN, T_EVAL], dtype=np.float64)
    data["q"], data["w"], data["viol64"] = q32, w32, viol
    for key in ("A1", "b1", "A2", "b2"):
        if raw[key] is not None:
            data["raw_" + key] = np.asarray(raw[key], dtype=np.float64)
    for key in ("P", "q", "r"):
        if len(raw[key]):
            data["raw_" + key] = np.stack([np.asarray(a, dtype=np.float64) for a in raw[key]])
    data["raw_y0"] = np.asarray(cs.y0, dtype=np.float64)
    os.makedirs(os.path.join(HERE, "dc3"), exist_ok=True)
    path = os.path.join(HERE, "dc3", f"dc3_{name}.npz")
    np.savez_compressed(path, **data)
    print(f"dc3_{name}: k={cs.k} n={cs.n} lr={args['lr']:g} eps={eps:.3e} steps train/eval "
          f"{int(data['steps64_train'])}/{int(data['steps64_eval'])} -> {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    only = set(sys.argv[1:])
    cases = [("cube", workloads.cube(), 2.0)]
    for index in range(15):
        cs = mg._example_cs(index)
        raw = mg._raw_from_ref_cs(cs)
        raw["y0"] = cs.y0
        cases.append((f"example_{index:02d}", raw, 2.0))
    cases.append(("c2", workloads.make_raw("c2", seed=2), 1.0))
    cases.append(("corridor", workloads.corridor_like(k=20, n_eq=5, m=30, n_quad=3, rank=2, seed=1), 1.0))
    for seed, (name, raw, scale) in enumerate(cases):
        if only and name not in only:
            continue
        _case(name, raw, scale, 900 + seed)


if __name__ == "__main__":
    main()
