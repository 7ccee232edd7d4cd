"""Host side of ``method='DC3'`` (completion + gradient correction, rayen/constraint_module.py:134-228 and :265-336).

``setup`` derives the reference's buffers (same names, same dtype rules, so its ``state_dict``s and pickles load),
``check_args`` validates ``args_DC3``, ``reference_forward`` is the reference's iteration in plain torch ops (host
tensors, the loud detour, and the comparator of ``scripts/dc3_bench.py``) and ``pack_arrays`` turns the CURRENT buffers
into the fp64 arrays ``ops.Dc3Pack`` uploads.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import utils

ARG_KEYS = ("lr", "momentum", "eps_converge", "max_steps_training", "max_steps_testing")
KERNEL_CHOICES = ("lane", "tile", "auto")      # the optional key args_DC3['kernel']; absent: 'lane'


def check_args(args_DC3):
    """``args_DC3`` needs the five keys of the reference; the two step limits must be finite integers >= 1 (documented
    deviation: the reference's commented-out ``float("inf")`` is refused -- the kernels size their scratch by it).  The
    optional key ``'kernel'`` is one of ``KERNEL_CHOICES``."""
    if args_DC3 is None:
        raise NotImplementedError("method 'DC3' needs args_DC3 (a dict with " + ", ".join(ARG_KEYS) + ")")
    missing = [key for key in ARG_KEYS if key not in args_DC3]
    if missing:
        raise ValueError(f"args_DC3 lacks {missing}; it needs " + ", ".join(ARG_KEYS))
    for key in ("max_steps_training", "max_steps_testing"):
        value = args_DC3[key]
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            if not (isinstance(value, float) and math.isfinite(value) and value == int(value)):
                raise ValueError(f"args_DC3['{key}'] must be a finite integer >= 1, got {value!r}")
        if int(value) < 1:
            raise ValueError(f"args_DC3['{key}'] must be a finite integer >= 1, got {value!r}")
    if "kernel" in args_DC3 and args_DC3["kernel"] not in KERNEL_CHOICES:
        raise ValueError(f"args_DC3['kernel'] must be one of {KERNEL_CHOICES}, got {args_DC3['kernel']!r}")


def kernel_choice(args_DC3):
    """``'lane'``, ``'tile'`` or ``'auto'``: what ``args_DC3`` asks for."""
    return (args_DC3 or {}).get("kernel", "lane")


def setup(module, cs):
    """Register the DC3 buffers and index sets on ``module`` (rayen/constraint_module.py:134-228)."""
    A2, b2 = utils.removeRedundantEquationsFromEqualitySystem(cs.A_E, cs.b_E)
    module.register_buffer("A2_DC3", torch.Tensor(A2))
    module.register_buffer("b2_DC3", torch.Tensor(b2))
    module.register_buffer("A1_DC3", torch.Tensor(cs.A_I))
    module.register_buffer("b1_DC3", torch.Tensor(cs.b_I))
    module.neq_DC3 = module.A2_DC3.shape[0]

    k = module.k
    if A2.shape[0] == 0:
        module.partial_vars = np.arange(k)
        module.other_vars = np.setdiff1d(np.arange(k), module.partial_vars)
    else:
        _, pivots_pos, _ = utils.rref(A2)
        module.other_vars = [pos[1] for pos in pivots_pos]          # the pivot columns are completed from the others
        module.partial_vars = np.setdiff1d(np.arange(k), module.other_vars)
    partial, other = _index_lists(module)

    A2p = module.A2_DC3[:, partial]
    A2o = module.A2_DC3[:, other]
    A2oi = torch.inverse(A2o)
    A1p = module.A1_DC3[:, partial]
    A1o = module.A1_DC3[:, other]
    module.register_buffer("A2oi", A2oi)
    module.register_buffer("A2p", A2p)
    module.register_buffer("A1_effective", A1p - A1o @ (A2oi @ A2p))
    module.register_buffer("b1_effective", module.b1_DC3 - A1o @ A2oi @ module.b2_DC3)

    # every quadratic restricted to the completion y[other] = A2oi (b2 - A2p p), at the default dtype (:189-224)
    n_quad, n_p, n_o = module.all_P.shape[0], len(partial), len(other)
    all_Pe = torch.zeros(n_quad, n_p, n_p)
    all_qe = torch.zeros(n_quad, n_p, 1)
    all_re = torch.zeros(n_quad, 1, 1)
    b2t = module.b2_DC3
    for i in range(n_quad):
        P, q, r = module.all_P[i], module.all_q[i], module.all_r[i]
        Po = P[np.ix_(other, other)].view(n_o, n_o)
        Pp = P[np.ix_(partial, partial)].view(n_p, n_p)
        Pop = P[np.ix_(other, partial)].view(n_o, n_p)
        qo, qp = q[other, 0:1], q[partial, 0:1]
        all_Pe[i] = 2 * (-A2p.T @ A2oi.T @ Pop + 0.5 * A2p.T @ A2oi.T @ Po @ A2oi @ A2p + 0.5 * Pp)
        all_qe[i] = (b2t.T @ A2oi.T @ Pop + qp.T - qo.T @ A2oi @ A2p - b2t.T @ A2oi.T @ Po @ A2oi @ A2p).T
        all_re[i] = qo.T @ A2oi @ b2t + 0.5 * b2t.T @ A2oi.T @ Po @ A2oi @ b2t + r
    module.register_buffer("all_P_effective", all_Pe)
    module.register_buffer("all_q_effective", all_qe)
    module.register_buffer("all_r_effective", all_re)


def _index_lists(module):
    return ([int(i) for i in module.partial_vars], [int(i) for i in module.other_vars])


def max_steps(module):
    key = "max_steps_training" if module.training else "max_steps_testing"      # (:282-285)
    return int(module.args_DC3[key])


def reference_forward(module, q, return_steps=False):
    """The reference's iteration (:269-336) with torch ops on ``q``'s device and dtype; differentiable by autograd.
    ``q [B, n, 1]``; returns ``y [B, k, 1]`` (and the number of steps taken)."""
    dt = q.dtype
    partial, other = _index_lists(module)
    buf = {name: getattr(module, name).to(dt) for name in
           ("A2oi", "A2p", "b2_DC3", "A1_effective", "b1_effective", "all_P_effective", "all_q_effective",
            "all_r_effective", "A1_DC3", "b1_DC3", "all_P", "all_q", "all_r")}
    args = module.args_DC3
    limit = max_steps(module)

    def quad(y, P, qv, r):
        return 0.5 * torch.transpose(y, 1, 2) @ P @ y + qv.T @ y + r

    y = torch.zeros((q.shape[0], module.k, 1), device=q.device, dtype=dt)
    y[:, partial, :] = q[:, :len(partial), :]
    y[:, other, :] = buf["A2oi"] @ (buf["b2_DC3"] - buf["A2p"] @ q[:, :len(partial), :])
    y_new, old_step, steps = y, 0, 0
    while True:
        yp = y_new[:, partial, :]
        A1e = buf["A1_effective"]
        grad = 2 * A1e.T @ torch.relu(A1e @ yp - buf["b1_effective"])
        for i in range(buf["all_P_effective"].shape[0]):
            Pe, qe, re = buf["all_P_effective"][i], buf["all_q_effective"][i], buf["all_r_effective"][i]
            grad = grad + 2 * (Pe @ yp + qe) @ torch.relu(quad(yp, Pe, qe, re))
        y_step = torch.zeros_like(y)
        y_step[:, partial, :] = grad
        y_step[:, other, :] = -buf["A2oi"] @ buf["A2p"] @ grad
        new_step = args["lr"] * y_step + args["momentum"] * old_step
        y_new = y_new - new_step
        old_step = new_step
        steps += 1

        stacked = buf["A1_DC3"] @ y_new - buf["b1_DC3"]
        for i in range(buf["all_P"].shape[0]):
            stacked = torch.cat((stacked, quad(y_new, buf["all_P"][i], buf["all_q"][i], buf["all_r"][i])), dim=1)
        if steps >= limit:
            break
        if stacked.numel() and torch.max(torch.relu(stacked)) < args["eps_converge"]:
            break
    return (y_new, steps) if return_steps else y_new


def pack_arrays(module):
    """fp64 arrays of the CURRENT buffers in the order ``rayen_dc3_pack_create`` takes them."""
    partial, other = _index_lists(module)
    d = lambda t: t.detach().double().cpu().numpy()           # noqa: E731
    n, no = len(partial), len(other)
    A2oi, A2p, b2 = d(module.A2oi), d(module.A2p), d(module.b2_DC3)
    C = -(A2oi @ A2p) if no else np.zeros((0, n))
    c0 = (A2oi @ b2).reshape(-1) if no else np.zeros((0,))
    nq = module.all_P_effective.shape[0]
    return dict(A1e=np.ascontiguousarray(d(module.A1_effective).reshape(-1, n)),
                b1e=np.ascontiguousarray(d(module.b1_effective).reshape(-1)),
                Pe=np.ascontiguousarray(d(module.all_P_effective).reshape(nq, n, n)),
                qe=np.ascontiguousarray(d(module.all_q_effective).reshape(nq, n)),
                re=np.ascontiguousarray(d(module.all_r_effective).reshape(nq)),
                C=np.ascontiguousarray(C.reshape(no, n)), c0=np.ascontiguousarray(c0),
                partial=np.asarray(partial, dtype=np.int32), other=np.asarray(other, dtype=np.int32),
                n=n, k=int(module.k))
