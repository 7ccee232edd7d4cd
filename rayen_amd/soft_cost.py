"""``SoftCost``: the soft cost and the violation of a batch against a set's ORIGINAL constraints, per sample.

What the reference's harness computes on the output of its baselines (examples/cost_computer.py:69-110: the training loss of
``UU``, ``UP`` and ``DC3``) and what every method's result is judged by (``ConvexConstraints.getResiduals``), as one module:

    cost[b]  = sum relu(g_r(y_b))^2 + sum (A2 y_b - b2)_r^2
    worst[b] = the largest g_r(y_b), with |A2 y_b - b2|_r counted;  which[b] = its index

over the inequality values ``g`` in the stacked order ``lin_ineq`` (``A1 y - b1``), ``quad`` (``0.5 y'Py + q'y + r``), ``soc``
(``||My + s|| - c'y - d``), ``lmi`` (``-lambda_min(F(y))``, one value), followed by the ``lin_eq`` rows.  ``cost`` is
differentiable in ``y``.

Tensors on a HIP device run ``rayen_amd/csrc/rayen_cost.hip`` through ``rayen_amd::soft_cost``: ONE launch reads ``y`` once
and writes ``cost``, ``worst``, ``which`` and -- when ``y`` requires a gradient -- ``d cost[b] / d y[b]``, so the backward is
``grad_out[:, None] * grad`` and nothing of size ``[B, rows]`` reaches memory.  A set's LMI runs on
``rayen_amd/csrc/rayen_cost_lmi.hip`` (a wave per sample: the matrix in LDS, its extreme eigenvalue by Householder + Sturm
multisection, the eigenvector only for samples outside): the only launch when the LMI is the set's only constraint, a second
one that adds to the first one's outputs otherwise.  The mirror below (the same formulas in plain torch ops, differentiated by
autograd; the LMI through ``torch.linalg.eigvalsh``) serves host tensors and sets the kernels refuse (one ``RuntimeWarning``;
an error under ``RAYEN_STRICT_HIP=1``).  16-bit inputs are computed in fp32.  A row with a NaN answers ``cost = worst = NaN``,
``which = -1``; no other row is touched.

``SoftCost(cs, kernel=...)`` chooses the route of device tensors.  ``'resident'`` (the default) is the above: the whole image
of the stacked rows in LDS, refused beyond 160 KiB.  ``'stream'`` runs ``rayen_amd/csrc/rayen_cost_stream.hip`` through
``rayen_amd::soft_cost_stream``: the same image cut into windows that a workgroup brings through LDS one after another, the
same arithmetic in the same order (bit for bit the resident result where both serve), for sets of any number of rows
(``k <= 64``).  ``'auto'`` takes the resident kernel wherever it serves at the input's dtype, else the streamed one, else the
mirror.  ``'tile64'`` runs ``rayen_amd/csrc/rayen_cost_tile64.hip`` through ``rayen_amd::soft_cost_tile64``: fp64 rows in
blocks of 16 stacked rows on the fp64 matrix cores, 32 samples per wave, the image through LDS in windows (``k <= 64``, any
number of rows); exact fp64 in another summation order than the lane kernels.  It is fp64 only: fp32 and 16-bit device rows
take the loud path to the mirror.  ``'auto'`` never chooses it.  Host tensors take the mirror under every value.
"""
from __future__ import annotations

import os
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import _lib

KERNELS = ("resident", "stream", "auto", "tile64")
_NAMES = ("A1", "b1", "P", "q", "r", "M", "s", "c", "d", "A2", "b2", "F")


def set_arrays(cs):
    """The set's constraints as contiguous fp64 arrays (what ``ops.CostPack`` uploads and the mirror evaluates):
    ``A1 [m1, k]``, ``b1 [m1]``, ``P [nq, k, k]``, ``q [nq, k]``, ``r [nq]``, ``M [sum rows, k]``, ``s [sum rows]``,
    ``c [nsoc, k]``, ``d [nsoc]``, ``soc_rows [nsoc]`` (int32), ``A2 [m2, k]``, ``b2 [m2]``, ``F [k + 1, r, r]`` (LMI) or empty."""
    k = int(cs.k)
    f = lambda a, *shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(*shape))          # noqa: E731
    out = dict(k=k)
    ineq, eq = cs.has_linear_ineq_constraints, cs.has_linear_eq_constraints
    out["A1"] = f(cs.lc.A1, -1, k) if ineq else np.zeros((0, k))
    out["b1"] = f(cs.lc.b1, -1) if ineq else np.zeros(0)
    out["A2"] = f(cs.lc.A2, -1, k) if eq else np.zeros((0, k))
    out["b2"] = f(cs.lc.b2, -1) if eq else np.zeros(0)
    qcs = list(cs.qcs) if cs.has_quadratic_constraints else []
    out["P"] = f([qc.P for qc in qcs], -1, k, k) if qcs else np.zeros((0, k, k))
    out["q"] = f([qc.q for qc in qcs], -1, k) if qcs else np.zeros((0, k))
    out["r"] = f([qc.r for qc in qcs], -1) if qcs else np.zeros(0)
    socs = list(cs.socs) if cs.has_soc_constraints else []
    out["M"] = f(np.concatenate([soc.M for soc in socs], axis=0), -1, k) if socs else np.zeros((0, k))
    out["s"] = f(np.concatenate([np.reshape(soc.s, -1) for soc in socs]), -1) if socs else np.zeros(0)
    out["c"] = f([soc.c for soc in socs], -1, k) if socs else np.zeros((0, k))
    out["d"] = f([soc.d for soc in socs], -1) if socs else np.zeros(0)
    out["soc_rows"] = np.asarray([soc.M.shape[0] for soc in socs], dtype=np.int32)
    out["F"] = f(np.stack(cs.lmic.all_F, axis=0), k + 1, *cs.lmic.all_F[0].shape) if cs.has_lmi_constraints else np.zeros((0, 0, 0))
    return out


# ------------------------------------------------------------------------------------------------------------------
# the mirror: the same formulas in plain torch ops
# ------------------------------------------------------------------------------------------------------------------

class Constants:
    """:func:`set_arrays` as torch tensors of one dtype on one device."""

    def __init__(self, tensors, soc_rows, dtype, device):
        for name in _NAMES:
            setattr(self, name, tensors[name].to(device=device, dtype=dtype))
        self.soc_rows = [int(r) for r in soc_rows]


def mirror_values(c, y):
    """``(g [B, n_ineq], e [B, m2])``: every inequality value in the stacked order, and the equality residuals."""
    B = y.shape[0]
    parts = [y @ c.A1.T - c.b1]
    if c.P.shape[0]:
        Py = torch.einsum("qij,bj->bqi", 0.5 * (c.P + c.P.transpose(1, 2)), y)
        parts.append(0.5 * torch.einsum("bqi,bi->bq", Py, y) + y @ c.q.T + c.r)
    if c.soc_rows:
        u = y @ c.M.T + c.s
        norms = [torch.linalg.vector_norm(piece, dim=1) for piece in torch.split(u, c.soc_rows, dim=1)]
        parts.append(torch.stack(norms, dim=1) - y @ c.c.T - c.d)
    if c.F.shape[0]:
        H = torch.einsum("ba,ajk->bjk", y, c.F[:-1]) + c.F[-1]
        lam = torch.full((B,), float("nan"), dtype=y.dtype, device=y.device)
        ok = torch.isfinite(y).all(dim=1)              # (eigvalsh raises on a NaN matrix: those rows answer NaN)
        if bool(ok.any()):
            lam = lam.masked_scatter(ok, torch.linalg.eigvalsh(H[ok])[:, 0])
        parts.append(-lam[:, None])
    return torch.cat(parts, dim=1), y @ c.A2.T - c.b2


def mirror(c, y):
    """``(cost [B], worst [B], which [B] int32)``; ``cost`` carries the autograd graph."""
    g, e = mirror_values(c, y)
    cost = torch.sum(torch.square(torch.relu(g)), dim=1) + torch.sum(torch.square(e), dim=1)
    cost = cost + 0.0 * (g.sum(dim=1) + e.sum(dim=1))        # (relu drops a NaN: put it back)
    with torch.no_grad():
        vals = torch.cat((g, e.abs()), dim=1)
        bad = torch.isnan(cost)
        worst, which = torch.max(torch.where(bad[:, None], torch.zeros_like(vals), vals), dim=1)
        worst = torch.where(bad, torch.full_like(worst, float("nan")), worst)
        which = torch.where(bad, torch.full_like(which, -1), which).to(torch.int32)
    return cost, worst, which


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------

class SoftCost(nn.Module):
    """``forward(y) -> cost [B]`` (differentiable in ``y``), ``violation(y) -> (worst [B], which [B] int32)`` for
    ``y [B, k, 1]`` or ``[B, k]``."""

    def __init__(self, cs, kernel="resident"):
        super().__init__()
        if kernel not in KERNELS:
            raise ValueError(f"rayen_amd: SoftCost(kernel=...) must be one of {KERNELS}, got {kernel!r}")
        self.kernel = kernel
        self.arrays = set_arrays(cs)           # fp64 numpy: what the packs are built from (picklable)
        self.k = int(cs.k)
        self.has_lmi_constraints = bool(cs.has_lmi_constraints)
        for name in _NAMES:
            self.register_buffer(name, torch.from_numpy(self.arrays[name].copy()))
        self._invalidate_packs()

    # ------------------------------------------------------------------ packs (rebuilt, never pickled)
    def _invalidate_packs(self):
        self.__dict__["_cost_packs"] = {}
        self.__dict__["_constants"] = {}
        self.__dict__["_unsupported"] = set()
        self.__dict__["_routes"] = {}

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._invalidate_packs()
        return out

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_cost_packs"], state["_constants"], state["_unsupported"], state["_routes"] = {}, {}, set(), {}
        return state

    def cost_pack(self, device):
        """(pack, pack_id) of the set on ``device`` (built on first use)."""
        from . import ops
        index = device.index if device.index is not None else torch.cuda.current_device()
        entry = self._cost_packs.get(index)
        if entry is None:
            pack = ops.CostPack(self.arrays, index)
            entry = self._cost_packs[index] = (pack, ops.register_pack(pack))
        return entry

    def constants(self, dtype, device):
        key = (dtype, str(device))
        c = self._constants.get(key)
        if c is None:
            tensors = {name: getattr(self, name) for name in _NAMES}
            c = self._constants[key] = Constants(tensors, self.arrays["soc_rows"], dtype, device)
        return c

    # ------------------------------------------------------------------ evaluation
    def _rows(self, y):
        y2 = torch.flatten(y, 1)
        if y2.shape[1] != self.k:
            raise RuntimeError(f"rayen_amd: expected y of shape [B, {self.k}] or [B, {self.k}, 1], got {tuple(y.shape)}")
        return y2

    def _mirror(self, y2):
        return mirror(self.constants(y2.dtype, y2.device), y2)

    def _route(self, pack, dtype):
        """``'resident'``, ``'stream'`` or ``'tile64'``: the route ``kernel`` sends device rows of ``dtype`` to (sizes alone decide).
        ``'auto'`` decides once per (device, dtype): the stream images are asked for at most once, at the default window."""
        if self.kernel != "auto":
            return self.kernel
        key = (pack.device_index, dtype)
        route = self._routes.get(key)
        if route is None:
            # (served by neither: 'resident', whose call refuses in the usual way)
            route = "resident" if pack.served(dtype) or not pack.stream_served(dtype) else "stream"
            self._routes[key] = route
        return route

    def _evaluate(self, y2, want_grad):
        """``(cost, worst, which)`` of fp32 / fp64 rows: the kernel where it serves, the mirror elsewhere."""
        if not y2.is_cuda or (y2.device.index, y2.dtype, self.kernel) in self._unsupported:
            return self._mirror(y2)
        try:
            from . import ops
            pack, pack_id = self.cost_pack(y2.device)
            route = self._route(pack, y2.dtype)
            if want_grad:
                op = {"stream": torch.ops.rayen_amd.soft_cost_stream, "tile64": torch.ops.rayen_amd.soft_cost_tile64}.get(
                    route, torch.ops.rayen_amd.soft_cost)
                cost, worst, which, _ = op(y2, pack_id, True)
            else:
                cost, worst, which, _ = ops.soft_cost_raw(y2.detach(), pack, False, kernel=route)
            return cost, worst, which
        except _lib.RayenError as err:
            if err.code != _lib.E_UNSUPPORTED or os.environ.get("RAYEN_STRICT_HIP", "0") == "1":
                raise
            warnings.warn(f"rayen_amd: no HIP kernel serves this set's soft cost ({err}); this module now evaluates the "
                          "same formulas in torch ops (rayen_amd/soft_cost.py) on " + str(y2.device), RuntimeWarning,
                          stacklevel=4)
            self._unsupported.add((y2.device.index, y2.dtype, self.kernel))
            return self._mirror(y2)

    def forward(self, y):
        y2 = self._rows(y)
        if y2.dtype not in (torch.float32, torch.float64):
            return self._evaluate(y2.float(), torch.is_grad_enabled() and y2.requires_grad)[0].to(y2.dtype)
        return self._evaluate(y2, torch.is_grad_enabled() and y2.requires_grad)[0]

    @torch.no_grad()
    def violation(self, y):
        y2 = self._rows(y)
        if y2.dtype not in (torch.float32, torch.float64):
            _, worst, which = self._evaluate(y2.float(), False)
            return worst.to(y2.dtype), which
        _, worst, which = self._evaluate(y2, False)
        return worst, which
