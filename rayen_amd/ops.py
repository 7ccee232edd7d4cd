"""``torch.library`` custom ops in front of the C ABI (``include/rayen_hip.h``).

``rayen_amd::ray_project(v, pack_id) -> (y, kappa, active)`` is the fused
replacement of ``forwardForRAYEN`` (rayen/constraint_module.py:468-474); it is
asynchronous on torch's current HIP stream and differentiable (the backward is
``rayen_amd::ray_project_bwd``, another HIP kernel).  PyTorch is used here for
device memory and the stream only.

These ops serve tensors on a HIP device only (anything else raises HERE; ``ConstraintModule`` sends host tensors
to ``rayen_amd/eager.py`` before it gets this far).  One detour exists and it is loud: a backward the kernels
decline with ``RAYEN_E_UNSUPPORTED`` (n beyond what they stage) is evaluated by autograd through the
packed torch evaluator on the same device, with a ``RuntimeWarning``; ``RAYEN_STRICT_HIP=1`` keeps the error.
"""
from __future__ import annotations

import ctypes
import os
import warnings
import weakref
from typing import Optional

import torch

from . import _lib

_packs = weakref.WeakValueDictionary()
_next_id = [1]


def register_pack(pack) -> int:
    pack_id = _next_id[0]
    _next_id[0] += 1
    _packs[pack_id] = pack
    return pack_id


def _pack(pack_id):
    pack = _packs.get(pack_id)
    if pack is None or pack.handle is None:
        raise RuntimeError(f"rayen_amd: constant pack {pack_id} no longer exists")
    return pack


def _check_input(v, pack):
    if not v.is_cuda:
        raise RuntimeError("rayen_amd: the projection runs on an MI355X (HIP) device only; got a "
                           f"{v.device} tensor. Move the module and its input to 'cuda'.")
    if v.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"rayen_amd: unsupported dtype {v.dtype} (float32 and float64 only)")
    if v.dim() != 2 or v.shape[1] < pack.consts.n:
        raise RuntimeError(f"rayen_amd: expected v of shape [B, >= {pack.consts.n}], got {tuple(v.shape)}")
    if v.device.index != pack.device_index:
        raise RuntimeError("rayen_amd: input and constant pack live on different devices")


def _dense_rows(t, width):
    """``t`` with unit column stride and rows that do not overlap (row stride >= ``width``), copied only where it has
    to be: ``row.expand(B, m)`` has row stride 0, and the one row of a ``[1, m]`` view may carry any stride.  The C ABI
    keeps refusing a leading dimension below ``width``."""
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < width):
        return t.contiguous()
    if t.shape[0] == 1 and t.stride(0) < width:
        return t.as_strided(t.shape, (t.shape[1], 1))        # one row: its stride addresses nothing
    return t


def _ptr(t):
    """Device address of a tensor as a plain int (ctypes converts it to ``void*``; building a ``c_void_p`` object per
    argument costs ~0.3 us each -- ten of them per call is a third of a small-batch forward's host time)."""
    return t.data_ptr() if t is not None else None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(index=None):
    """The caller's current HIP stream (a raw hipStream_t).  ``torch.cuda.current_stream().cuda_stream`` costs
    several microseconds of Python per call, which is most of a small-batch forward; the private accessor is what
    it ends in."""
    if _raw_stream is not None and index is not None:
        return _raw_stream(index) or None
    return torch.cuda.current_stream().cuda_stream or None


class _on_device:
    """``with torch.cuda.device(d)`` only when ``d`` is not already the current device."""
    __slots__ = ("index", "ctx")

    def __init__(self, device):
        self.index = device.index
        self.ctx = None

    def __enter__(self):
        if torch.cuda.current_device() != self.index:
            self.ctx = torch.cuda.device(self.index)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


_ENTRY = {}


def _entry(name):
    """The ctypes function object of an entry point (looked up once)."""
    fn = _ENTRY.get(name)
    if fn is None:
        fn = _ENTRY[name] = getattr(_lib.load(), name)
    return fn


_TYPED = {}


def _typed(name, dtype):
    """The entry point ``<name>_f32`` or ``<name>_f64`` that serves ``dtype``: one dictionary lookup per call (the name is
    put together, and looked up through ``_entry``, the first time only)."""
    fn = _TYPED.get((name, dtype))
    if fn is None:
        fn = _TYPED[(name, dtype)] = _entry(name + ("_f32" if dtype == torch.float32 else "_f64"))
    return fn


_FWD = {(torch.float32, False): "rayen_ray_project_f32", (torch.float64, False): "rayen_ray_project_f64",
        (torch.float32, True): "rayen_ray_project_generic_f32",
        (torch.float64, True): "rayen_ray_project_generic_f64"}
_FWD_OLD = {torch.float32: "rayen_ray_project_old_f32", torch.float64: "rayen_ray_project_old_f64"}
_BWD = {(torch.float32, False): "rayen_ray_project_bwd_f32", (torch.float64, False): "rayen_ray_project_bwd_f64",
        (torch.float32, True): "rayen_ray_project_old_bwd_f32",
        (torch.float64, True): "rayen_ray_project_old_bwd_f64"}


# Where the matrix-core kernels stop (n they keep in registers; include/rayen_hip.h) the forward
# goes GEMM + epilogue: T = v W_ext' on the vendor library (torch.mm -> hipBLASLt / rocBLAS on the caller's stream),
# then ONE hand-written kernel over T (rayen_wide.hip).  ``RAYEN_WIDE_ROUTE=0`` pins the lane-per-sample kernel.
_WIDE_MIN_N = {torch.float32: 129, torch.float64: 65}
# Sets = [linear rows] + one LMI on the workgroup-per-sample kernels (round 5) take the same route much earlier: S(v) for the
# whole batch is then ONE GEMM instead of every workgroup streaming all k generators for its sample.  Measured, B = 2 000, fp32,
# forward / backward ms, products against fused (profiles/bench/r05_lmi_products_ab.txt): r = 100 k = 50 0.84 / 0.99 against
# 0.89 / 1.14, k = 100 0.85 / 1.05 against 0.95 / 1.32, k = 1 000 1.01 / 1.31 against 2.34 / 7.72; r = 300 k = 100 14.9 / 17.3
# against 19.2 / 25.9, k = 500 15.6 / 18.5 against 37.8 / 63.2; a tie at k = 10.  T and the backward's C are [B, rows of W_ext]
# each: beyond _LMI_PRODUCTS_BYTES per matrix the fused kernels keep the batch (they need no scratch).
_LMI_WIDE_MIN_N = 32
_LMI_PRODUCTS_BYTES = 4 << 30


def _wide_route(v, pack, force_generic, old_head):
    if force_generic or old_head or os.environ.get("RAYEN_WIDE_ROUTE", "1") == "0":
        return None
    env = os.environ.get("RAYEN_WIDE_MIN_N")          # (developer A/B)
    has_lmi = any(seg.type == _lib.SEG_LMI for seg in pack.consts.segments)
    min_n = int(env) if env else (_LMI_WIDE_MIN_N if has_lmi else _WIDE_MIN_N[v.dtype])
    if pack.consts.n < min_n:
        return None
    Wt = pack.products_matrix(v.dtype)
    if Wt is not None and has_lmi and v.shape[0] * Wt.shape[1] * v.element_size() > _LMI_PRODUCTS_BYTES:
        return None
    return Wt


WIDE_KERNELS = ('products', 'fused', 'fused64')


def project_raw(v, pack, want_y=True, force_generic=False, want_active=True, old_head=False, out=None,
                want_kappa=True, wide_kernel='products', wide_samples=0):
    """Direct call of the C ABI on an existing ``DevicePack``; returns (y|None, kappa|None, active|None).

    ``old_head``: the ``RAYEN_old`` step rule; ``v`` then carries ``beta`` in column ``n``.
    ``out``: a ``[B, >=k]`` tensor (unit column stride) whose first ``k`` columns receive ``y`` -- e.g. this
    rank's rows of a gather buffer -- instead of a fresh allocation.
    ``wide_kernel``: what serves a call that takes the wide route (``_wide_route``): ``'products'`` -- the library GEMM and
    the epilogue over its products -- or ``'fused'`` -- ``rayen_ray_project_wide_fused_f32`` (rayen_wide_fused.hip): one
    launch, no GEMM and no products matrix; fp32, no LMI, n <= 1024, anything else is ``RAYEN_E_UNSUPPORTED`` -- or
    ``'fused64'`` -- its fp64 twin ``rayen_ray_project_wide_fused64_f64`` (rayen_wide_fused64.hip): fp64, no LMI, n <= 1024,
    anything else is ``RAYEN_E_UNSUPPORTED``.  No effect on a call that does not take the wide route.
    ``wide_samples`` (tests and measurements): the sample tile of ``'fused64'``, 16 or 32; 0 leaves it to the plan.  The bits
    of a row do not depend on it."""
    if wide_kernel not in WIDE_KERNELS:
        raise ValueError(f"wide_kernel must be one of {WIDE_KERNELS}, got {wide_kernel!r}")
    _check_input(v, pack)
    if old_head and v.shape[1] < pack.consts.n + 1:
        raise RuntimeError(f"rayen_amd: RAYEN_old needs {pack.consts.n + 1} input columns, got {v.shape[1]}")
    v = _dense_rows(v, pack.consts.n + (1 if old_head else 0))
    B = v.shape[0]
    k = pack.consts.k
    if out is not None:
        if (out.dim() != 2 or out.shape[0] != B or out.shape[1] < k or out.dtype != v.dtype
                or out.device != v.device or (B and out.stride(1) != 1)):
            raise RuntimeError(f"rayen_amd: out must be a [{B}, >={k}] {v.dtype} tensor on {v.device} with unit column stride")
        y = out
    else:
        y = torch.empty((B, k), dtype=v.dtype, device=v.device) if want_y else None
    kappa = torch.empty((B,), dtype=v.dtype, device=v.device) if want_kappa else None
    active = torch.empty((B, 2), dtype=torch.int32, device=v.device) if want_active else None
    Wt = _wide_route(v, pack, force_generic, old_head) if B else None
    with _on_device(v.device):
        if Wt is not None and wide_kernel == 'fused64':
            if v.dtype != torch.float64:
                code = _lib.E_UNSUPPORTED        # (the kernel is fp64 only; fp32 has 'fused')
            else:
                code = _entry("rayen_ray_project_wide_fused64_f64")(
                    pack.handle, _ptr(v), B, v.stride(0), _ptr(y), y.stride(0) if y is not None else k, _ptr(kappa),
                    _ptr(active), _ptr(pack.nan_flag), int(wide_samples), _stream(v.device.index))
            _lib.check(code, "rayen_ray_project_wide_fused64")
            return y, kappa, active
        if Wt is not None and wide_kernel == 'fused':
            if v.dtype != torch.float32:
                code = _lib.E_UNSUPPORTED        # (the fused kernel is fp32 only: rayen_wide_fused_served(pack, 1) == 0)
            else:
                code = _entry("rayen_ray_project_wide_fused_f32")(
                    pack.handle, _ptr(v), B, v.stride(0), _ptr(y), y.stride(0) if y is not None else k, _ptr(kappa),
                    _ptr(active), _ptr(pack.nan_flag), _stream(v.device.index))
            _lib.check(code, "rayen_ray_project_wide_fused")
            return y, kappa, active
        if Wt is not None:
            n = pack.consts.n
            prods = torch.mm(v if v.shape[1] == n else v[:, :n], Wt)         # [B, rows of W_ext]: the library GEMM
            fn = _typed("rayen_ray_project_from_products", v.dtype)
            code = fn(pack.handle, _ptr(prods), prods.stride(0), _ptr(v), B, v.stride(0), _ptr(y),
                      y.stride(0) if y is not None else k, _ptr(kappa), _ptr(active), _ptr(pack.nan_flag),
                      _stream(v.device.index))
        else:
            fn = _entry(_FWD_OLD[v.dtype] if old_head else _FWD[(v.dtype, bool(force_generic))])
            code = fn(pack.handle, _ptr(v), B, v.stride(0) if B else pack.consts.n, _ptr(y),
                      y.stride(0) if (y is not None and B) else k,
                      _ptr(kappa), _ptr(active), _ptr(pack.nan_flag), _stream(v.device.index))
    _lib.check(code, "rayen_ray_project")
    return y, kappa, active


@torch.library.custom_op("rayen_amd::ray_project", mutates_args=())
def ray_project(v: torch.Tensor, pack_id: int, need_active: bool, old_head: bool = False) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``need_active``: also record which constraint set kappa (only the backward reads it; without
    it the kernels skip the arg-max bookkeeping and ``active`` comes back empty).
    ``old_head``: the ``RAYEN_old`` step rule (``v[:, n]`` is ``beta``)."""
    y, kappa, active = project_raw(v, _pack(pack_id), want_active=need_active, old_head=old_head)
    if active is None:
        active = torch.empty((0, 2), dtype=torch.int32, device=v.device)
    return y, kappa, active


@ray_project.register_fake
def _(v, pack_id, need_active, old_head=False):
    pack = _pack(pack_id)
    B = v.shape[0]
    return (v.new_empty((B, pack.consts.k)), v.new_empty((B,)),
            v.new_empty((B if need_active else 0, 2), dtype=torch.int32))


@torch.library.custom_op("rayen_amd::ray_project_wide_fused", mutates_args=())
def ray_project_wide_fused(v: torch.Tensor, pack_id: int, need_active: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``rayen_amd::ray_project`` with ``wide_kernel='fused'``: wide sets on rayen_wide_fused.hip (a call that does not take
    the wide route runs what ``ray_project`` runs).  Its backward is ``ray_project``'s: the products route consumes this
    forward's ``kappa`` and ``active``."""
    y, kappa, active = project_raw(v, _pack(pack_id), want_active=need_active, wide_kernel='fused')
    if active is None:
        active = torch.empty((0, 2), dtype=torch.int32, device=v.device)
    return y, kappa, active


@ray_project_wide_fused.register_fake
def _(v, pack_id, need_active):
    pack = _pack(pack_id)
    B = v.shape[0]
    return (v.new_empty((B, pack.consts.k)), v.new_empty((B,)),
            v.new_empty((B if need_active else 0, 2), dtype=torch.int32))


WIDE_BACKWARDS = ('products', 'fused', 'fused64')
# the fused wide backwards: route -> (dtype it serves, workspace query, entry point, takes `wide_samples`, name in errors)
_WIDE_FUSED_BWD = {
    'fused': (torch.float32, "rayen_wide_fused_bwd_workspace_bytes", "rayen_ray_project_wide_fused_bwd_f32", False,
              "rayen_ray_project_wide_fused_bwd"),
    'fused64': (torch.float64, "rayen_wide_fused_bwd64_workspace_bytes", "rayen_ray_project_wide_fused_bwd_f64", True,
                "rayen_ray_project_wide_fused_bwd64"),
}


def backward_raw(v, kappa, active, grad_y, pack, old_head=False, force_generic=False, bucketed=True,
                 wide_backward='products', group=True, wide_samples=0):
    """Direct call of the backward entry points; ``force_generic`` pins the lane-per-sample kernel
    where ``rayen_ray_project_bwd_f32/_f64`` would pick the matrix-core one.  ``bucketed``: hand the library the
    scratch buffer it asks for (``rayen_bwd_workspace_bytes_f32``) so that it may group the samples by active
    constraint and walk only that constraint's tiles; ``False`` pins the plain walk (same results).
    ``wide_backward``: what serves a call that takes the wide route (``_wide_route``): ``'products'`` -- two library GEMMs
    around the coefficient kernel of rayen_wide.hip -- or ``'fused'`` -- ``rayen_ray_project_wide_fused_bwd_f32``
    (rayen_wide_fused_bwd.hip): one launch over the active constraints' rows, neither T nor C; fp32, no LMI, n <= 1024,
    anything else is ``RAYEN_E_UNSUPPORTED`` -- or ``'fused64'`` -- its fp64 twin ``rayen_ray_project_wide_fused_bwd_f64``
    (rayen_wide_fused_bwd64.hip): fp64, no LMI, n <= 1024, anything else is ``RAYEN_E_UNSUPPORTED``.  No effect on a call
    that does not take the wide route.  ``group`` (developer flag of the fused routes): hand the library the workspace with
    which it groups the rows by active constraint; ``False`` pins batch order (same bits).  ``wide_samples`` (tests and
    measurements): the sample tile of ``'fused64'``, 16 or 32; 0 leaves it to the plan.  The bits of a row do not depend on
    it."""
    if wide_backward not in WIDE_BACKWARDS:
        raise ValueError(f"wide_backward must be one of {WIDE_BACKWARDS}, got {wide_backward!r}")
    _check_input(v, pack)
    v = _dense_rows(v, pack.consts.n + (1 if old_head else 0))
    grad_y = grad_y.contiguous()
    B = v.shape[0]
    # the kernels write the first n (+1 for the old head) columns of every row; wider inputs keep zeros
    used = pack.consts.n + (1 if old_head else 0)
    grad_v = torch.empty_like(v) if v.shape[1] == used else torch.zeros_like(v)
    name = _BWD[(v.dtype, bool(old_head))]
    if force_generic:
        if old_head:
            raise RuntimeError("force_generic selects between the two RAYEN backward kernels only")
        name = "rayen_ray_project_bwd_generic_f32" if v.dtype == torch.float32 else "rayen_ray_project_bwd_generic_f64"
    Wt = _wide_route(v, pack, force_generic, old_head) if B else None
    if Wt is not None and wide_backward in _WIDE_FUSED_BWD:
        # one launch over the active constraints' rows: each route serves its own precision alone
        dtype, ws_fn, entry, takes_samples, what = _WIDE_FUSED_BWD[wide_backward]
        with _on_device(v.device):
            if v.dtype != dtype:
                code = _lib.E_UNSUPPORTED        # ('fused' is fp32 only, 'fused64' fp64 only)
            else:
                lib = _lib.load()
                ws_bytes = int(getattr(lib, ws_fn)(pack.handle, B)) if group else 0
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=v.device) if ws_bytes > 0 else None   # (caching allocator)
                tile = (int(wide_samples),) if takes_samples else ()
                code = getattr(lib, entry)(
                    pack.handle, _ptr(v), B, v.stride(0), _ptr(kappa), _ptr(active), _ptr(grad_y), grad_y.stride(0),
                    _ptr(grad_v), grad_v.stride(0), _ptr(ws), ws_bytes, *tile, _stream(v.device.index))
        _lib.check(code, what)
        return grad_v
    if Wt is not None:
        # wide sets: T = v W_ext' again (one GEMM), the coefficient kernel, grad_v = C W_ext (+ s g): rayen_wide.hip
        n, k = pack.consts.n, pack.consts.k
        identity = bool(pack.consts.out_identity)
        with _on_device(v.device):
            prods = torch.mm(v if v.shape[1] == n else v[:, :n], Wt)
            coeff = torch.empty_like(prods)
            gs = torch.empty((B, k), dtype=v.dtype, device=v.device) if identity else None
            fn = _typed("rayen_ray_project_bwd_coefficients", v.dtype)
            code = fn(pack.handle, _ptr(prods), prods.stride(0), _ptr(v), B, v.stride(0), _ptr(kappa), _ptr(active),
                      _ptr(grad_y), grad_y.stride(0), _ptr(coeff), coeff.stride(0), _ptr(gs), _stream(v.device.index))
            _lib.check(code, "rayen_ray_project_bwd_coefficients")
            core = torch.addmm(gs, coeff, Wt.t()) if identity else torch.mm(coeff, Wt.t())
        if v.shape[1] == n:
            return core
        grad_v[:, :n] = core
        return grad_v
    with _on_device(v.device):
        lib = _lib.load()
        ws_bytes = 0
        tag = "f32" if v.dtype == torch.float32 else "f64"
        if bucketed and not old_head and not force_generic and B:
            ws_bytes = int(getattr(lib, "rayen_bwd_workspace_bytes_" + tag)(pack.handle, B))
        if ws_bytes > 0:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=v.device)   # (torch's caching allocator: no hipMalloc)
            code = getattr(lib, "rayen_ray_project_bwd_ws_" + tag)(pack.handle, _ptr(v), B, v.stride(0), _ptr(kappa), _ptr(active),
                                                                   _ptr(grad_y), grad_y.shape[1], _ptr(grad_v), grad_v.stride(0),
                                                                   _ptr(ws), ws_bytes, _stream(v.device.index))
        else:
            code = getattr(lib, name)(pack.handle, _ptr(v), B, v.stride(0) if B else pack.consts.n,
                                      _ptr(kappa), _ptr(active), _ptr(grad_y), grad_y.shape[1],
                                      _ptr(grad_v), grad_v.stride(0) if B else pack.consts.n,
                                      _stream(v.device.index))
    _lib.check(code, "rayen_ray_project_bwd")
    return grad_v


@torch.library.custom_op("rayen_amd::ray_project_bwd", mutates_args=())
def ray_project_bwd(v: torch.Tensor, kappa: torch.Tensor, active: torch.Tensor,
                    grad_y: torch.Tensor, pack_id: int, old_head: bool = False) -> torch.Tensor:
    return backward_raw(v, kappa, active, grad_y, _pack(pack_id), old_head)


def _bwd_or_detour(v, kappa, active, grad_y, pack_id, old_head, wide_backward='products'):
    """The HIP backward; where the kernels decline the shape (``RAYEN_E_UNSUPPORTED``), autograd through the packed
    torch evaluator on the same device -- loudly, once per pack and route.  Called from the autograd formulas (NOT from
    inside the custom op: below the dispatcher's autograd key nothing would be recorded).  A refusal of
    ``wide_backward='fused'`` or ``'fused64'`` is remembered per dtype and route: later calls go to the evaluator without
    asking again."""
    fused = wide_backward in ('fused', 'fused64')
    if fused and (v.dtype, wide_backward) in _pack(pack_id).__dict__.get("_refused_bwd", ()):
        return _eager_backward(_pack(pack_id), v, grad_y, old_head)
    try:
        if wide_backward == 'fused64':
            return torch.ops.rayen_amd.ray_project_bwd_wide_fused64(v, kappa, active, grad_y, pack_id)
        if fused:
            return torch.ops.rayen_amd.ray_project_bwd_wide_fused(v, kappa, active, grad_y, pack_id)
        return torch.ops.rayen_amd.ray_project_bwd(v, kappa, active, grad_y, pack_id, old_head)
    except _lib.RayenError as err:
        if err.code != _lib.E_UNSUPPORTED or os.environ.get("RAYEN_STRICT_HIP", "0") == "1":
            raise
        pack = _pack(pack_id)
        warned = "_warned_bwd_wide_" + wide_backward if fused else "_warned_bwd"
        if not pack.__dict__.get(warned):
            warnings.warn(f"rayen_amd: no HIP backward kernel serves this constraint set ({err}); gradients come from "
                          "autograd through the packed torch evaluator (rayen_amd/eager.py) on " + str(v.device),
                          RuntimeWarning, stacklevel=2)
            pack.__dict__[warned] = True
        if fused:
            pack.__dict__.setdefault("_refused_bwd", set()).add((v.dtype, wide_backward))
        return _eager_backward(pack, v, grad_y, old_head)


def _eager_backward(pack, v, grad_y, old_head):
    from . import eager
    key = ("_eager", v.dtype)
    ev = pack.__dict__.get(key)
    if ev is None:
        ev = pack.__dict__[key] = eager.PackedEvaluator(pack.consts, v.dtype, v.device)
    with torch.enable_grad():
        leaf = v.detach().clone().requires_grad_(True)
        y, _ = ev.project(leaf, old_head=old_head)
        (grad_v,) = torch.autograd.grad(y, leaf, grad_y.to(y.dtype))
    return grad_v


@ray_project_bwd.register_fake
def _(v, kappa, active, grad_y, pack_id, old_head=False):
    return torch.empty_like(v)


def _setup_context(ctx, inputs, output):
    v, pack_id, need_active, old_head = inputs
    ctx.old_head = old_head
    if not need_active:
        raise RuntimeError("rayen_amd::ray_project was called with need_active=False on an input that "
                           "requires grad")
    _, kappa, active = output
    ctx.pack_id = pack_id
    ctx.save_for_backward(v, kappa, active)


def _backward(ctx, grad_y, grad_kappa, grad_active):
    v, kappa, active = ctx.saved_tensors
    if grad_y is None:
        return torch.zeros_like(v), None, None, None
    return (_bwd_or_detour(v, kappa, active, grad_y, ctx.pack_id, ctx.old_head), None, None, None)


ray_project.register_autograd(_backward, setup_context=_setup_context)


def _wide_fused_setup_context(ctx, inputs, output):
    v, pack_id, need_active = inputs
    _setup_context(ctx, (v, pack_id, need_active, False), output)


def _wide_fused_backward(ctx, grad_y, grad_kappa, grad_active):
    return _backward(ctx, grad_y, grad_kappa, grad_active)[:3]


ray_project_wide_fused.register_autograd(_wide_fused_backward, setup_context=_wide_fused_setup_context)


@torch.library.custom_op("rayen_amd::ray_project_bwd_wide_fused", mutates_args=())
def ray_project_bwd_wide_fused(v: torch.Tensor, kappa: torch.Tensor, active: torch.Tensor, grad_y: torch.Tensor,
                               pack_id: int) -> torch.Tensor:
    """``rayen_amd::ray_project_bwd`` with ``wide_backward='fused'``: wide sets on rayen_wide_fused_bwd.hip (a call that
    does not take the wide route runs what ``ray_project_bwd`` runs)."""
    return backward_raw(v, kappa, active, grad_y, _pack(pack_id), wide_backward='fused')


@ray_project_bwd_wide_fused.register_fake
def _(v, kappa, active, grad_y, pack_id):
    return torch.empty_like(v)


@torch.library.custom_op("rayen_amd::ray_project_bwd_wide_fused64", mutates_args=())
def ray_project_bwd_wide_fused64(v: torch.Tensor, kappa: torch.Tensor, active: torch.Tensor, grad_y: torch.Tensor,
                                 pack_id: int) -> torch.Tensor:
    """``rayen_amd::ray_project_bwd`` with ``wide_backward='fused64'``: wide sets in fp64 on rayen_wide_fused_bwd64.hip (a
    call that does not take the wide route runs what ``ray_project_bwd`` runs)."""
    return backward_raw(v, kappa, active, grad_y, _pack(pack_id), wide_backward='fused64')


@ray_project_bwd_wide_fused64.register_fake
def _(v, kappa, active, grad_y, pack_id):
    return torch.empty_like(v)


@torch.library.custom_op("rayen_amd::ray_project_wide", mutates_args=())
def ray_project_wide(v: torch.Tensor, pack_id: int, need_active: bool, wide_kernel: str,
                     wide_backward: str) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``rayen_amd::ray_project`` with both choices of the wide route spelled out: the forward by ``wide_kernel``, the
    backward (``rayen_amd::ray_project_bwd``, ``rayen_amd::ray_project_bwd_wide_fused`` or ``..._wide_fused64``) by ``wide_backward`` -- it consumes
    ``kappa`` and ``active`` of whichever forward made them."""
    if wide_backward not in WIDE_BACKWARDS:
        raise ValueError(f"wide_backward must be one of {WIDE_BACKWARDS}, got {wide_backward!r}")
    y, kappa, active = project_raw(v, _pack(pack_id), want_active=need_active, wide_kernel=wide_kernel)
    if active is None:
        active = torch.empty((0, 2), dtype=torch.int32, device=v.device)
    return y, kappa, active


@ray_project_wide.register_fake
def _(v, pack_id, need_active, wide_kernel, wide_backward):
    pack = _pack(pack_id)
    B = v.shape[0]
    return (v.new_empty((B, pack.consts.k)), v.new_empty((B,)),
            v.new_empty((B if need_active else 0, 2), dtype=torch.int32))


def _wide_setup_context(ctx, inputs, output):
    v, pack_id, need_active, _, wide_backward = inputs
    _setup_context(ctx, (v, pack_id, need_active, False), output)
    ctx.wide_backward = wide_backward


def _wide_backward(ctx, grad_y, grad_kappa, grad_active):
    v, kappa, active = ctx.saved_tensors
    if grad_y is None:
        return torch.zeros_like(v), None, None, None, None
    return (_bwd_or_detour(v, kappa, active, grad_y, ctx.pack_id, False, ctx.wide_backward), None, None, None, None)


ray_project_wide.register_autograd(_wide_backward, setup_context=_wide_setup_context)


# ------------------------------------------------------------------------------------------------
# mapper + projection in one launch (rayen/constraint_module.py:525 followed by :468-474)
# ------------------------------------------------------------------------------------------------

def mapper_fusable(x, weight, bias, pack):
    """Can ``ray_project_mapped`` serve this call?  (fp32, contiguous rows, and a fused form for this pack and input
    width: weights read in place by the exact-fp32 family, or through their split-operand image by the default one.)"""
    if not (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 2
            and weight.dim() == 2 and weight.shape[0] == pack.consts.n and x.shape[1] == weight.shape[1]
            and weight.stride(1) == 1
            and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous()))):
        return False
    mode = pack.mapper_mode(weight.shape[1])
    if mode == 1:
        return weight.is_contiguous() and weight.data_ptr() % 16 == 0
    return mode == 2


@torch.library.custom_op("rayen_amd::ray_project_mapped", mutates_args=())
def ray_project_mapped(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], pack_id: int,
                       need_grad: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(y, kappa, active, v)`` with ``v = x weight' + bias`` evaluated inside the projection kernel.

    ``need_grad``: also write ``v`` and the active-constraint record (the backward's inputs); without it
    ``v`` never reaches memory and both come back empty."""
    pack = _pack(pack_id)
    if not mapper_fusable(x, weight, bias, pack):
        raise RuntimeError("rayen_amd::ray_project_mapped: unsupported mapper (check ops.mapper_fusable first)")
    if x.device.index != pack.device_index:
        raise RuntimeError("rayen_amd: input and constant pack live on different devices")
    if x.stride(1) != 1:
        x = x.contiguous()
    B, in_dim = x.shape
    k, n = pack.consts.k, pack.consts.n
    y = torch.empty((B, k), dtype=x.dtype, device=x.device)
    kappa = torch.empty((B,), dtype=x.dtype, device=x.device)
    active = torch.empty((B if need_grad else 0, 2), dtype=torch.int32, device=x.device)
    v = torch.empty((B if need_grad else 0, n), dtype=x.dtype, device=x.device)
    with _on_device(x.device):
        stream = _stream(x.device.index)
        if pack.mapper_mode(in_dim) == 2:
            image = pack.mapper_image(weight, bias, stream)
            code = _lib.load().rayen_ray_project_mapped_image_f32(
                pack.handle, _ptr(x), B, x.stride(0) if B else in_dim, in_dim, _ptr(image),
                _ptr(v) if need_grad else None, n, _ptr(y), k, _ptr(kappa),
                _ptr(active) if need_grad else None, _ptr(pack.nan_flag), stream)
        else:
            code = _lib.load().rayen_ray_project_mapped_f32(
                pack.handle, _ptr(x), B, x.stride(0) if B else in_dim, in_dim, _ptr(weight), weight.stride(0),
                _ptr(bias), _ptr(v) if need_grad else None, n, _ptr(y), k, _ptr(kappa),
                _ptr(active) if need_grad else None, _ptr(pack.nan_flag), stream)
    _lib.check(code, "rayen_ray_project_mapped")
    return y, kappa, active, v


@ray_project_mapped.register_fake
def _(x, weight, bias, pack_id, need_grad):
    pack = _pack(pack_id)
    B = x.shape[0]
    rows = B if need_grad else 0
    return (x.new_empty((B, pack.consts.k)), x.new_empty((B,)),
            x.new_empty((rows, 2), dtype=torch.int32), x.new_empty((rows, pack.consts.n)))


def _mapped_setup_context(ctx, inputs, output):
    x, weight, bias, pack_id, need_grad = inputs
    if not need_grad:
        raise RuntimeError("rayen_amd::ray_project_mapped was called with need_grad=False on inputs that "
                           "require grad")
    _, kappa, active, v = output
    ctx.pack_id = pack_id
    ctx.has_bias = bias is not None
    ctx.save_for_backward(x, weight, v, kappa, active)


def _mapped_backward(ctx, grad_y, grad_kappa, grad_active, grad_v_out):
    x, weight, v, kappa, active = ctx.saved_tensors
    if grad_y is None:
        return None, None, None, None, None
    # d y / d v on the HIP backward kernel; the three mapper products are plain GEMMs (rocBLAS via torch)
    grad_v = _bwd_or_detour(v, kappa, active, grad_y, ctx.pack_id, False)
    grad_x = grad_v @ weight if ctx.needs_input_grad[0] else None
    grad_w = grad_v.t() @ x if ctx.needs_input_grad[1] else None
    grad_b = grad_v.sum(0) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
    return grad_x, grad_w, grad_b, None, None


ray_project_mapped.register_autograd(_mapped_backward, setup_context=_mapped_setup_context)


# ... and in fp64: the mapper in front of the fp64 matrix-core forward (include/rayen_hip_mapped64.h), weights read in place

def mapper_fusable64(x, weight, bias, pack):
    """Can ``ray_project_mapped64`` serve this call?  (fp64 device tensors, ``weight [n, in_dim]`` with unit column stride
    -- any row stride: every load is one double --, and a pack the fp64 matrix-core forward serves, ``in_dim <= 512``.)"""
    if not (x.is_cuda and weight.is_cuda and x.dtype == torch.float64 and weight.dtype == torch.float64 and x.dim() == 2
            and weight.dim() == 2 and weight.shape[0] == pack.consts.n and x.shape[1] == weight.shape[1]
            and weight.shape[1] >= 1 and weight.stride(1) == 1 and weight.stride(0) >= weight.shape[1]
            and (bias is None or (bias.is_cuda and bias.dtype == torch.float64 and bias.is_contiguous()
                                  and bias.shape == (pack.consts.n,)))):
        return False
    return pack.mapper_mode64(weight.shape[1]) == 1


@torch.library.custom_op("rayen_amd::ray_project_mapped64", mutates_args=())
def ray_project_mapped64(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], pack_id: int,
                         need_grad: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(y, kappa, active, v)`` of ``ray_project_mapped`` in fp64: ``v = x weight' + bias`` formed on the fp64 matrix
    cores inside the projection kernel.

    ``need_grad``: also write ``v`` and the active-constraint record (the backward's inputs); without it
    ``v`` never reaches memory and both come back empty."""
    pack = _pack(pack_id)
    if not mapper_fusable64(x, weight, bias, pack):
        raise RuntimeError("rayen_amd::ray_project_mapped64: unsupported mapper (check ops.mapper_fusable64 first)")
    if x.device.index != pack.device_index:
        raise RuntimeError("rayen_amd: input and constant pack live on different devices")
    B, in_dim = x.shape
    if x.stride(1) != 1 or (B > 1 and x.stride(0) < in_dim):
        x = x.contiguous()
    k, n = pack.consts.k, pack.consts.n
    y = torch.empty((B, k), dtype=x.dtype, device=x.device)
    kappa = torch.empty((B,), dtype=x.dtype, device=x.device)
    active = torch.empty((B if need_grad else 0, 2), dtype=torch.int32, device=x.device)
    v = torch.empty((B if need_grad else 0, n), dtype=x.dtype, device=x.device)
    if B == 0:
        return y, kappa, active, v           # (empty tensors have no address to hand to the library)
    with _on_device(x.device):
        code = _lib.load().rayen_ray_project_mapped_f64(
            pack.handle, _ptr(x), B, x.stride(0) if B > 1 else in_dim, in_dim, _ptr(weight), weight.stride(0),
            _ptr(bias), _ptr(v) if need_grad else None, n, _ptr(y), k, _ptr(kappa),
            _ptr(active) if need_grad else None, _ptr(pack.nan_flag), _stream(x.device.index))
    _lib.check(code, "rayen_ray_project_mapped64")
    return y, kappa, active, v


@ray_project_mapped64.register_fake
def _(x, weight, bias, pack_id, need_grad):
    pack = _pack(pack_id)
    B = x.shape[0]
    rows = B if need_grad else 0
    return (x.new_empty((B, pack.consts.k)), x.new_empty((B,)),
            x.new_empty((rows, 2), dtype=torch.int32), x.new_empty((rows, pack.consts.n)))


def _mapped64_setup_context(ctx, inputs, output):
    if not inputs[4]:
        raise RuntimeError("rayen_amd::ray_project_mapped64 was called with need_grad=False on inputs that "
                           "require grad")
    _mapped_setup_context(ctx, inputs, output)


# (the same formula: d y / d v on the HIP backward kernel from the saved v, the three mapper products in torch)
ray_project_mapped64.register_autograd(_mapped_backward, setup_context=_mapped64_setup_context)


# ------------------------------------------------------------------------------------------------
# What the side layers below (Bar, DC3, Euclidean projection, soft cost) share: each owns an opaque pack of the library
# (rayen_<layer>_pack_create / _destroy: an fp32 and an fp64 image on one device), tests its input rows the same way and
# calls a pair of typed entry points (``_typed`` above); two of them size a scratch buffer first.
# ------------------------------------------------------------------------------------------------

class _SidePack:
    """Owner of one opaque pack of the library on one device.  Immutable, so a captured graph may keep using it."""
    _layer = None             # "bar", "dc3", ...: rayen_<layer>_pack_create and rayen_<layer>_pack_destroy
    handle = None

    def _create(self, device_index, *args):
        self.device_index = int(device_index)
        handle = ctypes.c_void_p()
        name = f"rayen_{self._layer}_pack_create"
        with torch.cuda.device(self.device_index):
            _lib.check(_entry(name)(*args, ctypes.byref(handle)), name)
        self.handle = handle

    def close(self):
        if self.handle:
            _entry(f"rayen_{self._layer}_pack_destroy")(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass


# layer -> (how its op is called, how its pack is called) in the messages of _check_rows
_LAYER_NAMES = {"bar": ("the Bar layer's HIP op", "Bar pack"), "dc3": ("the DC3 layer's HIP op", "DC3 pack"),
                "proj": ("the projection's HIP op", "projection pack"), "cost": ("the soft-cost HIP op", "cost pack")}


def _check_rows(t, width, pack, what, layer):
    """``t`` (called ``what``) is a ``[B, >= width]`` fp32 / fp64 tensor on the HIP device of ``pack``, or this raises."""
    if not t.is_cuda:
        raise RuntimeError(f"rayen_amd: {_LAYER_NAMES[layer][0]} runs on an MI355X (HIP) device only; got a "
                           f"{t.device} tensor")
    if t.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"rayen_amd: unsupported dtype {t.dtype} (float32 and float64 only)")
    if t.dim() != 2 or t.shape[1] < width:
        raise RuntimeError(f"rayen_amd: expected {what} of shape [B, >= {width}], got {tuple(t.shape)}")
    if t.device.index != pack.device_index:
        raise RuntimeError(f"rayen_amd: input and {_LAYER_NAMES[layer][1]} live on different devices")


def _host_ptr(x):
    """Address of a numpy array for the library; an empty one is passed as NULL."""
    return x.ctypes.data if x.size else None


def _workspace(pack, t, backward, max_steps=None, tile=False):
    """``(scratch tensor, its size for the library)`` of a DC3 call (``max_steps`` given) or a projection call on the rows
    of ``t``, as ``rayen_*_workspace_bytes`` sizes it (``tile``: false for the lane / wave kernels, else the tile kernel's
    name, ``'tile'`` or ``'tile64'``); refused beyond the layer's ``*_MAX_WORKSPACE_BYTES`` (read
    here, at call time)."""
    B, f64 = t.shape[0], int(t.dtype == torch.float64)
    if max_steps is not None:
        limit, extra = DC3_MAX_WORKSPACE_BYTES, 0
        if tile:
            name = "rayen_dc3_tile64_workspace_bytes" if tile == "tile64" else "rayen_dc3_tile_workspace_bytes"
            nbytes = int(_entry(name)(pack.handle, B, int(max_steps), int(backward)))
        else:
            name = "rayen_dc3_workspace_bytes"
            nbytes = int(_entry(name)(pack.handle, B, int(max_steps), f64, int(backward)))
    else:
        limit, extra = PROJ_MAX_WORKSPACE_BYTES, B * pack.m * t.element_size()   # (v*)
        if tile:
            name = "rayen_proj_tile64_workspace_bytes" if tile == "tile64" else "rayen_proj_tile_workspace_bytes"
            nbytes = int(_entry(name)(pack.handle, B, int(backward)))
        else:
            name = "rayen_proj_workspace_bytes"
            nbytes = int(_entry(name)(pack.handle, B, f64, int(backward)))
    if nbytes < 0:
        raise RuntimeError(f"rayen_amd: {name} refused its arguments")
    if nbytes + extra > limit:
        call = "backward" if backward else "forward"
        if max_steps is not None:
            raise RuntimeError(f"rayen_amd: the DC3 {call} of {B} rows x {max_steps} steps needs {nbytes} bytes of scratch, more "
                               f"than ops.DC3_MAX_WORKSPACE_BYTES = {limit}; lower the step limit or split the batch")
        raise RuntimeError(f"rayen_amd: the projection {call} of {B} rows x {pack.m} cone rows needs {nbytes + extra} bytes of "
                           f"scratch, more than ops.PROJ_MAX_WORKSPACE_BYTES = {limit}; split the batch")
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=t.device), nbytes


# ------------------------------------------------------------------------------------------------
# method='Bar' (rayen/constraint_module.py:479-486): y = G [softmax(q_v); |q_r|] + yp on rayen_bar.hip
# ------------------------------------------------------------------------------------------------

class BarPack(_SidePack):
    """Owner of one ``RayenBarPack*``: fp32 and fp64 images of ``G = NA_E [V R]`` (k x (nv + nr)) and ``yp`` on one
    device, plus the NaN flag its forward raises."""
    _layer = "bar"

    def __init__(self, G, yp, nv, nr, device_index):
        import numpy as np
        self.k, self.nv, self.nr = int(G.shape[0]), int(nv), int(nr)
        G = np.ascontiguousarray(G, dtype=np.float64)
        yp = np.ascontiguousarray(np.reshape(yp, -1), dtype=np.float64)
        self._create(device_index, G.ctypes.data, yp.ctypes.data, self.k, self.nv, self.nr)
        self.nan_flag = torch.zeros(1, dtype=torch.int32, device=f"cuda:{self.device_index}")
        # (asked once, here: a module's 'auto' route then looks the answer up, also while torch.compile traces it)
        self._resident = {dtype: bool(_entry("rayen_bar_resident_served")(self.handle, int(dtype == torch.float64)))
                          for dtype in (torch.float32, torch.float64)}

    @property
    def width(self):
        return self.nv + self.nr

    def resident_served(self, dtype):
        """Do ``rayen_bar_forward_*`` / ``rayen_bar_backward_*`` (the image of G resident in LDS) serve this pack at
        ``dtype``?  (The streamed kernels serve every pack.)"""
        return self._resident[dtype]


BAR_KERNELS = ("resident", "stream")


def _bar_entry(kernel, direction, dtype):
    """The typed entry point of a Bar call on ``kernel``."""
    if kernel == "resident":
        return _typed("rayen_bar_" + direction, dtype)
    if kernel == "stream":
        return _typed("rayen_bar_stream_" + direction, dtype)
    raise ValueError(f"rayen_amd: kernel must be one of {BAR_KERNELS}, got {kernel!r}")


def bar_forward_raw(q, pack, want_rowstat=True, kernel='resident', window_bytes=0):
    """``(y [B, k], rowstat [B] | None)`` through ``rayen_bar_forward_*`` (``kernel='resident'``: the image of G in LDS) or
    ``rayen_bar_stream_forward_*`` (``kernel='stream'``: the image streamed through LDS in windows of ``window_bytes``, 0 =
    the default; the same bits wherever both serve the pack); ``rowstat`` is the per-row log-sum-exp of the vertex logits
    (the backward's input)."""
    fn = _bar_entry(kernel, "forward", q.dtype)
    _check_rows(q, pack.width, pack, "q", "bar")
    q = _dense_rows(q, pack.width)
    B = q.shape[0]
    y = torch.empty((B, pack.k), dtype=q.dtype, device=q.device)
    rowstat = torch.empty((B,), dtype=q.dtype, device=q.device) if want_rowstat else None
    extra = () if kernel == "resident" else (int(window_bytes),)
    with _on_device(q.device):
        code = fn(pack.handle, _ptr(q), B, q.stride(0) if B else pack.width, _ptr(y), pack.k, _ptr(rowstat),
                  _ptr(pack.nan_flag), *extra, _stream(q.device.index))
    _lib.check(code, "rayen_bar_forward" if kernel == "resident" else "rayen_bar_stream_forward")
    return y, rowstat


def bar_backward_raw(q, rowstat, grad_y, pack, kernel='resident', window_bytes=0):
    """``grad_q`` (same shape as ``q``; columns beyond ``nv + nr`` are zero) through ``rayen_bar_backward_*`` or, with
    ``kernel='stream'``, ``rayen_bar_stream_backward_*``."""
    fn = _bar_entry(kernel, "backward", q.dtype)
    _check_rows(q, pack.width, pack, "q", "bar")
    q = _dense_rows(q, pack.width).contiguous()
    grad_y = grad_y.to(q.dtype).contiguous()
    rowstat = rowstat.contiguous()
    B = q.shape[0]
    grad_q = torch.empty_like(q) if q.shape[1] == pack.width else torch.zeros_like(q)
    extra = () if kernel == "resident" else (int(window_bytes),)
    with _on_device(q.device):
        code = fn(pack.handle, _ptr(q), q.shape[1], _ptr(rowstat), _ptr(grad_y), B, _ptr(grad_q), *extra,
                  _stream(q.device.index))
    _lib.check(code, "rayen_bar_backward" if kernel == "resident" else "rayen_bar_stream_backward")
    return grad_q


@torch.library.custom_op("rayen_amd::bar_project", mutates_args=())
def bar_project(q: torch.Tensor, pack_id: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``(y [B, k], rowstat [B])``: the Bar layer's forward on torch's current stream."""
    return bar_forward_raw(q, _pack(pack_id))


@bar_project.register_fake
def _(q, pack_id):
    pack = _pack(pack_id)
    return q.new_empty((q.shape[0], pack.k)), q.new_empty((q.shape[0],))


@torch.library.custom_op("rayen_amd::bar_project_bwd", mutates_args=())
def bar_project_bwd(q: torch.Tensor, rowstat: torch.Tensor, grad_y: torch.Tensor, pack_id: int) -> torch.Tensor:
    return bar_backward_raw(q, rowstat, grad_y, _pack(pack_id))


@bar_project_bwd.register_fake
def _(q, rowstat, grad_y, pack_id):
    return torch.empty_like(q)


def _bar_setup_context(ctx, inputs, output):
    q, pack_id = inputs
    ctx.pack_id = pack_id
    ctx.save_for_backward(q, output[1])


def _bar_backward(ctx, grad_y, grad_rowstat):
    q, rowstat = ctx.saved_tensors
    if grad_y is None:
        return None, None
    return torch.ops.rayen_amd.bar_project_bwd(q, rowstat, grad_y, ctx.pack_id), None


bar_project.register_autograd(_bar_backward, setup_context=_bar_setup_context)


# the same layer on the streamed kernels (rayen_bar_stream.hip); window_bytes = 0: the default window
@torch.library.custom_op("rayen_amd::bar_project_stream", mutates_args=())
def bar_project_stream(q: torch.Tensor, pack_id: int, window_bytes: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``(y [B, k], rowstat [B])``: the Bar layer's forward on the streamed kernel, on torch's current stream."""
    return bar_forward_raw(q, _pack(pack_id), kernel="stream", window_bytes=window_bytes)


@bar_project_stream.register_fake
def _(q, pack_id, window_bytes):
    pack = _pack(pack_id)
    return q.new_empty((q.shape[0], pack.k)), q.new_empty((q.shape[0],))


@torch.library.custom_op("rayen_amd::bar_project_stream_bwd", mutates_args=())
def bar_project_stream_bwd(q: torch.Tensor, rowstat: torch.Tensor, grad_y: torch.Tensor, pack_id: int,
                           window_bytes: int) -> torch.Tensor:
    return bar_backward_raw(q, rowstat, grad_y, _pack(pack_id), kernel="stream", window_bytes=window_bytes)


@bar_project_stream_bwd.register_fake
def _(q, rowstat, grad_y, pack_id, window_bytes):
    return torch.empty_like(q)


def _bar_stream_setup_context(ctx, inputs, output):
    q, pack_id, window_bytes = inputs
    ctx.pack_id, ctx.window_bytes = pack_id, window_bytes
    ctx.save_for_backward(q, output[1])


def _bar_stream_backward(ctx, grad_y, grad_rowstat):
    q, rowstat = ctx.saved_tensors
    if grad_y is None:
        return None, None, None
    return torch.ops.rayen_amd.bar_project_stream_bwd(q, rowstat, grad_y, ctx.pack_id, ctx.window_bytes), None, None


bar_project_stream.register_autograd(_bar_stream_backward, setup_context=_bar_stream_setup_context)


# ------------------------------------------------------------------------------------------------
# method='DC3' (rayen/constraint_module.py:265-336): completion + T gradient-correction steps on rayen_dc3.hip
# ------------------------------------------------------------------------------------------------

# The backward keeps the recomputed trajectory [max_steps][n][B]; beyond this it refuses (train with fewer correction steps
# or smaller batches: the reference's autograd graph holds several times as much).
DC3_MAX_WORKSPACE_BYTES = 8 << 30


class Dc3Pack(_SidePack):
    """Owner of one ``RayenDc3Pack*``: fp32 and fp64 images of the effective forms (``rayen_amd/dc3.py::pack_arrays``) on one
    device, plus the NaN flag its forward raises.  The tile kernels' images (fp32: rayen_dc3_tile.hip, fp64:
    rayen_dc3_tile64.hip) are uploaded each on the first call that asks for ``kernel='tile'`` / ``'tile64'``: a user who
    never does allocates nothing for them on the device.  Until both are settled the pack keeps a reference to the host
    arrays it was built from (no copy; released once both images are up)."""
    _layer = "dc3"

    def __init__(self, arrays, device_index):
        a, ptr = arrays, _host_ptr
        self.n, self.k = int(a["n"]), int(a["k"])
        self.inequalities = int(a["A1e"].shape[0]) + int(a["Pe"].shape[0])
        self._create(device_index, ptr(a["A1e"]), ptr(a["b1e"]), int(a["A1e"].shape[0]), ptr(a["Pe"]), ptr(a["qe"]),
                     ptr(a["re"]), int(a["Pe"].shape[0]), ptr(a["C"]), ptr(a["c0"]), ptr(a["partial"]), ptr(a["other"]),
                     self.n, self.k)
        self.nan_flag = torch.zeros(1, dtype=torch.int32, device=f"cuda:{self.device_index}")
        self._arrays = arrays      # the host arrays: what rayen_dc3_tile*_pack_set read, should they ever be called
        self._tile_set = set()     # of "rayen_dc3_tile_pack_set" / "rayen_dc3_tile64_pack_set": the uploads settled
        self._lane_served = {}

    def _tile_image(self, setter):
        if setter not in self._tile_set:
            a, ptr = self._arrays, _host_ptr
            with torch.cuda.device(self.device_index):
                _lib.check(_entry(setter)(self.handle, ptr(a["A1e"]), ptr(a["b1e"]), ptr(a["Pe"]), ptr(a["qe"]),
                                          ptr(a["re"]), ptr(a["C"]), ptr(a["c0"])), setter)
            self._tile_set.add(setter)
            if len(self._tile_set) == 2:
                self._arrays = None

    def tile_images(self):
        """Upload the fp32 tile kernels' image (once; not while a stream is capturing)."""
        self._tile_image("rayen_dc3_tile_pack_set")

    def tile64_images(self):
        """Upload the fp64 tile kernels' image (once; not while a stream is capturing)."""
        self._tile_image("rayen_dc3_tile64_pack_set")


DC3_KERNELS = ("lane", "tile")                  # the kernels that take fp32 input
DC3_KERNELS_F64 = ("lane", "tile64")            # ... and fp64 input ('tile64' is not in DC3_KERNELS: it refuses fp32)
_DC3_KERNEL_NAMES = ("lane", "tile", "tile64")


def _dc3_entry(direction, kernel, dtype, pack):
    """The library entry of ``kernel``: ``'lane'`` is rayen_dc3.hip (one lane per row, the image in LDS), ``'tile'``
    rayen_dc3_tile.hip (32 rows per workgroup on the matrix cores; fp32 only: an fp64 call is refused with
    ``E_UNSUPPORTED``), ``'tile64'`` rayen_dc3_tile64.hip (16 rows per workgroup on the fp64 matrix cores; fp64 only: an
    fp32 call is refused with ``E_UNSUPPORTED``)."""
    if kernel not in _DC3_KERNEL_NAMES:
        raise ValueError(f"kernel must be one of {_DC3_KERNEL_NAMES}, got {kernel!r}")
    if kernel == "lane":
        return _typed(f"rayen_dc3_{direction}", dtype)
    if kernel == "tile64":
        if dtype != torch.float64:
            raise _lib.RayenError(_lib.E_UNSUPPORTED, f"rayen_dc3_tile64_{direction}")
        pack.tile64_images()
        return _entry(f"rayen_dc3_tile64_{direction}_f64")
    if dtype != torch.float32:
        raise _lib.RayenError(_lib.E_UNSUPPORTED, f"rayen_dc3_tile_{direction}")
    pack.tile_images()
    return _entry(f"rayen_dc3_tile_{direction}_f32")


def dc3_forward_raw(q, pack, lr, momentum, eps, max_steps, kernel='lane'):
    """``(y [B, k], steps [1] int32)`` through ``rayen_dc3_forward_*`` (``kernel='tile'``: ``rayen_dc3_tile_forward_f32``;
    ``kernel='tile64'``: ``rayen_dc3_tile64_forward_f64``); ``steps`` is the batch-global number of steps."""
    _check_rows(q, pack.n, pack, "q", "dc3")
    entry = _dc3_entry("forward", kernel, q.dtype, pack)
    q = _dense_rows(q, pack.n)
    B = q.shape[0]
    if pack.inequalities == 0:
        # the reference never meets its stop rule on a set without inequalities (dc3.reference_forward: nothing is
        # stacked) and runs to the limit; the kernels' violations are all 0 there, and 0 < 0 is false
        eps = 0.0
    y = torch.empty((B, pack.k), dtype=q.dtype, device=q.device)
    steps = torch.empty((1,), dtype=torch.int32, device=q.device)
    with _on_device(q.device):
        ws, nbytes = _workspace(pack, q, False, max_steps, tile=kernel != "lane" and kernel)
        code = entry(
            pack.handle, _ptr(q), B, q.stride(0) if B else pack.n, _ptr(y), pack.k, float(lr), float(momentum),
            float(eps), int(max_steps), _ptr(steps), _ptr(ws), nbytes, _ptr(pack.nan_flag), _stream(q.device.index))
    _lib.check(code, "rayen_dc3_forward")
    return y, steps


def dc3_backward_raw(q, steps, grad_y, pack, lr, momentum, max_steps, kernel='lane'):
    """``grad_q`` (same shape as ``q``; columns beyond ``n`` are zero) through ``rayen_dc3_backward_*`` (``kernel='tile'``:
    ``rayen_dc3_tile_backward_f32``; ``kernel='tile64'``: ``rayen_dc3_tile64_backward_f64``); ``steps`` may come from any
    kernel's forward at the same precision."""
    _check_rows(q, pack.n, pack, "q", "dc3")
    entry = _dc3_entry("backward", kernel, q.dtype, pack)
    q = _dense_rows(q, pack.n)
    grad_y = grad_y.to(q.dtype).contiguous()
    B = q.shape[0]
    grad_q = torch.empty((B, q.shape[1]), dtype=q.dtype, device=q.device) if q.shape[1] == pack.n else \
        torch.zeros((B, q.shape[1]), dtype=q.dtype, device=q.device)
    with _on_device(q.device):
        ws, nbytes = _workspace(pack, q, True, max_steps, tile=kernel != "lane" and kernel)
        code = entry(
            pack.handle, _ptr(q), B, q.stride(0) if B else pack.n, _ptr(grad_y), pack.k, _ptr(grad_q),
            grad_q.stride(0) if B else pack.n, float(lr), float(momentum), int(max_steps), _ptr(steps), _ptr(ws), nbytes,
            _stream(q.device.index))
    _lib.check(code, "rayen_dc3_backward")
    return grad_q


def dc3_lane_served(pack, dtype):
    """Does the lane kernel (rayen_dc3.hip) stage this pack's image at ``dtype``?  Asked with an empty batch: no kernel is
    launched.  The library answers ``E_UNSUPPORTED`` before it touches the device; where it serves the pack, the empty call
    clears its few bytes of scratch and the step count (two ``hipMemsetAsync`` on the current stream).  Asked once per
    pack and dtype (the answer is remembered on the pack): not to be asked first while a stream is capturing."""
    if dtype not in pack._lane_served:
        try:
            dc3_forward_raw(torch.empty((0, pack.n), dtype=dtype, device=f"cuda:{pack.device_index}"), pack, 0.0, 0.0, 0.0, 1)
            pack._lane_served[dtype] = True
        except _lib.RayenError as err:
            if err.code != _lib.E_UNSUPPORTED:
                raise
            pack._lane_served[dtype] = False
    return pack._lane_served[dtype]


def dc3_tile_served(pack):
    """Does the tile kernel serve this pack (its envelope: ``Dc3TileLayout32::served()`` in rayen_dc3_tile_image.h)?  Uploads the
    tile image on first use (an allocation and a copy: not while a stream is capturing)."""
    pack.tile_images()
    return bool(_entry("rayen_dc3_tile_served")(pack.handle))


def dc3_tile64_served(pack):
    """Does the fp64 tile kernel serve this pack (its envelope: ``Dc3TileLayout64::served()`` in rayen_dc3_tile_image.h)?
    Uploads the fp64 tile image on first use (an allocation and a copy: not while a stream is capturing)."""
    pack.tile64_images()
    return bool(_entry("rayen_dc3_tile64_served")(pack.handle))


@torch.library.custom_op("rayen_amd::dc3_project", mutates_args=())
def dc3_project(q: torch.Tensor, pack_id: int, lr: float, momentum: float, eps: float,
                max_steps: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``(y [B, k], steps [1] int32)``: the DC3 layer's forward on torch's current stream."""
    return dc3_forward_raw(q, _pack(pack_id), lr, momentum, eps, max_steps)


@dc3_project.register_fake
def _(q, pack_id, lr, momentum, eps, max_steps):
    pack = _pack(pack_id)
    return q.new_empty((q.shape[0], pack.k)), q.new_empty((1,), dtype=torch.int32)


@torch.library.custom_op("rayen_amd::dc3_project_bwd", mutates_args=())
def dc3_project_bwd(q: torch.Tensor, steps: torch.Tensor, grad_y: torch.Tensor, pack_id: int, lr: float,
                    momentum: float, max_steps: int) -> torch.Tensor:
    return dc3_backward_raw(q, steps, grad_y, _pack(pack_id), lr, momentum, max_steps)


@dc3_project_bwd.register_fake
def _(q, steps, grad_y, pack_id, lr, momentum, max_steps):
    return torch.empty_like(q)


def _dc3_setup_context(ctx, inputs, output):
    q, pack_id, lr, momentum, eps, max_steps = inputs
    ctx.pack_id, ctx.lr, ctx.momentum, ctx.max_steps = pack_id, lr, momentum, max_steps
    ctx.save_for_backward(q, output[1])


def _dc3_backward(ctx, grad_y, grad_steps):
    q, steps = ctx.saved_tensors
    if grad_y is None:
        return None, None, None, None, None, None
    return (torch.ops.rayen_amd.dc3_project_bwd(q, steps, grad_y, ctx.pack_id, ctx.lr, ctx.momentum, ctx.max_steps),
            None, None, None, None, None)


dc3_project.register_autograd(_dc3_backward, setup_context=_dc3_setup_context)


@torch.library.custom_op("rayen_amd::dc3_project_tile", mutates_args=())
def dc3_project_tile(q: torch.Tensor, pack_id: int, lr: float, momentum: float, eps: float,
                     max_steps: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``dc3_project`` on the tile kernel (rayen_dc3_tile.hip)."""
    return dc3_forward_raw(q, _pack(pack_id), lr, momentum, eps, max_steps, kernel="tile")


@dc3_project_tile.register_fake
def _(q, pack_id, lr, momentum, eps, max_steps):
    pack = _pack(pack_id)
    return q.new_empty((q.shape[0], pack.k)), q.new_empty((1,), dtype=torch.int32)


@torch.library.custom_op("rayen_amd::dc3_project_tile_bwd", mutates_args=())
def dc3_project_tile_bwd(q: torch.Tensor, steps: torch.Tensor, grad_y: torch.Tensor, pack_id: int, lr: float,
                         momentum: float, max_steps: int) -> torch.Tensor:
    return dc3_backward_raw(q, steps, grad_y, _pack(pack_id), lr, momentum, max_steps, kernel="tile")


@dc3_project_tile_bwd.register_fake
def _(q, steps, grad_y, pack_id, lr, momentum, max_steps):
    return torch.empty_like(q)


def _dc3_tile_backward(ctx, grad_y, grad_steps):
    q, steps = ctx.saved_tensors
    if grad_y is None:
        return None, None, None, None, None, None
    return (torch.ops.rayen_amd.dc3_project_tile_bwd(q, steps, grad_y, ctx.pack_id, ctx.lr, ctx.momentum, ctx.max_steps),
            None, None, None, None, None)


dc3_project_tile.register_autograd(_dc3_tile_backward, setup_context=_dc3_setup_context)


@torch.library.custom_op("rayen_amd::dc3_project_tile64", mutates_args=())
def dc3_project_tile64(q: torch.Tensor, pack_id: int, lr: float, momentum: float, eps: float,
                       max_steps: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``dc3_project`` in fp64 on the fp64 tile kernel (rayen_dc3_tile64.hip)."""
    return dc3_forward_raw(q, _pack(pack_id), lr, momentum, eps, max_steps, kernel="tile64")


@dc3_project_tile64.register_fake
def _(q, pack_id, lr, momentum, eps, max_steps):
    pack = _pack(pack_id)
    return q.new_empty((q.shape[0], pack.k)), q.new_empty((1,), dtype=torch.int32)


@torch.library.custom_op("rayen_amd::dc3_project_tile64_bwd", mutates_args=())
def dc3_project_tile64_bwd(q: torch.Tensor, steps: torch.Tensor, grad_y: torch.Tensor, pack_id: int, lr: float,
                           momentum: float, max_steps: int) -> torch.Tensor:
    return dc3_backward_raw(q, steps, grad_y, _pack(pack_id), lr, momentum, max_steps, kernel="tile64")


@dc3_project_tile64_bwd.register_fake
def _(q, steps, grad_y, pack_id, lr, momentum, max_steps):
    return torch.empty_like(q)


def _dc3_tile64_backward(ctx, grad_y, grad_steps):
    q, steps = ctx.saved_tensors
    if grad_y is None:
        return None, None, None, None, None, None
    return (torch.ops.rayen_amd.dc3_project_tile64_bwd(q, steps, grad_y, ctx.pack_id, ctx.lr, ctx.momentum, ctx.max_steps),
            None, None, None, None, None)


dc3_project_tile64.register_autograd(_dc3_tile64_backward, setup_context=_dc3_setup_context)


# ------------------------------------------------------------------------------------------------
# Euclidean projection onto the set (the PP / UP baselines, rayen_amd/projection.py) on rayen_proj.hip
# ------------------------------------------------------------------------------------------------

# v* [B, m] plus the state between launches; beyond this the op refuses (split the batch)
PROJ_MAX_WORKSPACE_BYTES = 8 << 30


class ProjPack(_SidePack):
    """Owner of one ``RayenProjPack*``: fp32 and fp64 images of a ``projection.Program`` on one device.  The fp64 tile
    kernel's images are uploaded on request (``tile64_images``): until then the pack keeps the host arrays."""
    _layer = "proj"

    def __init__(self, arrays, device_index):
        a, ptr = arrays, _host_ptr
        self.n, self.m = int(a["n"]), int(a["m"])
        self._arrays = {k: a[k] for k in ("G", "h", "Kinv", "w0", "soc_rows")}
        self._create(device_index, ptr(a["G"]), ptr(a["h"]), ptr(a["Kinv"]), ptr(a["w0"]), self.n, self.m, int(a["m_lin"]),
                     ptr(a["soc_rows"]), int(a["soc_rows"].size), float(a["rho"]), float(a["sigma"]), float(a["alpha"]))
        if int(a.get("psd_dim", 0)):          # the set's LMI: the last rows of G are its PSD block, svec
            with torch.cuda.device(self.device_index):
                _lib.check(_entry("rayen_proj_pack_set_psd")(self.handle, int(a["psd_row0"]), int(a["psd_dim"])),
                           "rayen_proj_pack_set_psd")

    def tile64_images(self):
        """Upload the fp64 tile kernel's images (once; an allocation and a copy: not while a stream is capturing).  A
        program outside its envelope gets none."""
        if self._arrays is not None:
            a, ptr = self._arrays, _host_ptr
            with torch.cuda.device(self.device_index):
                _lib.check(_entry("rayen_proj_tile64_pack_set")(self.handle, ptr(a["G"]), ptr(a["h"]), ptr(a["Kinv"]),
                                                                ptr(a["w0"]), ptr(a["soc_rows"]), int(a["soc_rows"].size)),
                           "rayen_proj_tile64_pack_set")
            self._arrays = None


PROJ_KERNELS = ("wave", "tile")                 # the kernels that take fp32 input
PROJ_KERNELS_F64 = ("wave", "tile64")           # ... and fp64 input ('tile64' is not in PROJ_KERNELS: it refuses fp32)
_PROJ_KERNEL_NAMES = ("wave", "tile", "tile64")


def _proj_entry(direction, kernel, dtype, pack):
    """The library entry of ``kernel``: ``'wave'`` is rayen_proj.hip (wave per sample), ``'tile'`` rayen_proj_tile.hip (32
    samples per workgroup on the matrix cores; fp32 only: an fp64 call is refused with ``E_UNSUPPORTED``), ``'tile64'``
    rayen_proj_tile64.hip (16 samples per workgroup on the fp64 matrix cores; fp64 only: an fp32 call is refused with
    ``E_UNSUPPORTED``)."""
    if kernel not in _PROJ_KERNEL_NAMES:
        raise ValueError(f"kernel must be one of {_PROJ_KERNEL_NAMES}, got {kernel!r}")
    if kernel == "wave":
        return _typed(f"rayen_proj_{direction}", dtype)
    if kernel == "tile64":
        if dtype != torch.float64:
            raise _lib.RayenError(_lib.E_UNSUPPORTED, f"rayen_proj_tile64_{direction}")
        pack.tile64_images()
        return _entry(f"rayen_proj_tile64_{direction}_f64")
    if dtype != torch.float32:
        raise _lib.RayenError(_lib.E_UNSUPPORTED, f"rayen_proj_tile_{direction}")
    return _entry(f"rayen_proj_tile_{direction}_f32")


def proj_forward_raw(q, pack, max_iters, eps, kernel='wave'):
    """``(z [B, n], iters [B] int32, vstar [B, m])`` through ``rayen_proj_forward_*`` (``kernel='tile'``:
    ``rayen_proj_tile_forward_f32``; ``kernel='tile64'``: ``rayen_proj_tile64_forward_f64``)."""
    _check_rows(q, pack.n, pack, "q", "proj")
    entry = _proj_entry("forward", kernel, q.dtype, pack)
    q = _dense_rows(q, pack.n)
    B = q.shape[0]
    z = torch.empty((B, pack.n), dtype=q.dtype, device=q.device)
    iters = torch.empty((B,), dtype=torch.int32, device=q.device)
    vstar = torch.empty((B, pack.m), dtype=q.dtype, device=q.device)
    with _on_device(q.device):
        ws, nbytes = _workspace(pack, q, False, tile=kernel != "wave" and kernel)
        code = entry(
            pack.handle, _ptr(q), B, q.stride(0) if B else pack.n, _ptr(z), pack.n, _ptr(iters), _ptr(vstar),
            float(eps), int(max_iters), _ptr(ws), nbytes, _stream(q.device.index))
    _lib.check(code, "rayen_proj_forward")
    return z, iters, vstar


def proj_backward_raw(grad_z, vstar, iters, pack, max_iters, eps, kernel='wave'):
    """``grad_q [B, n] = J grad_z`` row by row through ``rayen_proj_backward_*`` (``kernel='tile'``:
    ``rayen_proj_tile_backward_f32``; ``kernel='tile64'``: ``rayen_proj_tile64_backward_f64``); ``vstar`` and ``iters`` may
    come from any kernel's forward at the same precision."""
    _check_rows(grad_z, pack.n, pack, "grad_z", "proj")
    entry = _proj_entry("backward", kernel, grad_z.dtype, pack)
    g = _dense_rows(grad_z, pack.n)
    vstar, iters = vstar.contiguous(), iters.contiguous()
    B = g.shape[0]
    grad_q = torch.empty((B, pack.n), dtype=g.dtype, device=g.device)
    with _on_device(g.device):
        ws, nbytes = _workspace(pack, g, True, tile=kernel != "wave" and kernel)
        code = entry(
            pack.handle, _ptr(g), B, g.stride(0) if B else pack.n, _ptr(vstar), _ptr(iters), _ptr(grad_q), pack.n,
            float(eps), int(max_iters), _ptr(ws), nbytes, _stream(g.device.index))
    _lib.check(code, "rayen_proj_backward")
    return grad_q


@torch.library.custom_op("rayen_amd::euclid_project", mutates_args=())
def euclid_project(q: torch.Tensor, pack_id: int, max_iters: int,
                   eps: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(z [B, n], iters [B] int32, vstar [B, m])``: the Euclidean projection on torch's current stream."""
    return proj_forward_raw(q, _pack(pack_id), max_iters, eps)


@euclid_project.register_fake
def _(q, pack_id, max_iters, eps):
    pack = _pack(pack_id)
    B = q.shape[0]
    return q.new_empty((B, pack.n)), q.new_empty((B,), dtype=torch.int32), q.new_empty((B, pack.m))


@torch.library.custom_op("rayen_amd::euclid_project_bwd", mutates_args=())
def euclid_project_bwd(grad_z: torch.Tensor, vstar: torch.Tensor, iters: torch.Tensor, pack_id: int, max_iters: int,
                       eps: float) -> torch.Tensor:
    return proj_backward_raw(grad_z, vstar, iters, _pack(pack_id), max_iters, eps)


@euclid_project_bwd.register_fake
def _(grad_z, vstar, iters, pack_id, max_iters, eps):
    return grad_z.new_empty((grad_z.shape[0], _pack(pack_id).n))


def _proj_setup_context(ctx, inputs, output):
    q, pack_id, max_iters, eps = inputs
    ctx.pack_id, ctx.max_iters, ctx.eps, ctx.width = pack_id, max_iters, eps, q.shape[1]
    ctx.save_for_backward(output[2], output[1])


def _proj_backward(ctx, grad_z, grad_iters, grad_vstar):
    vstar, iters = ctx.saved_tensors
    if grad_z is None:
        return None, None, None, None
    pack = _pack(ctx.pack_id)
    grad_q = torch.ops.rayen_amd.euclid_project_bwd(grad_z.to(vstar.dtype), vstar, iters, ctx.pack_id, ctx.max_iters,
                                                    ctx.eps)
    if ctx.width > pack.n:          # columns of q beyond n are not read
        grad_q = torch.nn.functional.pad(grad_q, (0, ctx.width - pack.n))
    return grad_q, None, None, None


euclid_project.register_autograd(_proj_backward, setup_context=_proj_setup_context)


def proj_wave_served(pack, dtype):
    """Does the wave kernel (rayen_proj.hip) stage this pack's program at ``dtype``?  Asked with an empty batch: the
    library answers ``E_UNSUPPORTED`` before it would launch anything."""
    with torch.cuda.device(pack.device_index):
        code = _typed("rayen_proj_forward", dtype)(pack.handle, None, 0, pack.n, None, pack.n, None, None, 1e-6, 1, None, 0,
                                                   None)
    if code == _lib.E_UNSUPPORTED:
        return False
    _lib.check(code, "rayen_proj_forward")
    return True


def proj_tile_served(pack):
    """Does the tile kernel hold this pack's program (its envelope: ``tile_served()`` in rayen_proj_tile.hip)?"""
    return bool(_entry("rayen_proj_tile_served")(pack.handle))


@torch.library.custom_op("rayen_amd::euclid_project_tile", mutates_args=())
def euclid_project_tile(q: torch.Tensor, pack_id: int, max_iters: int,
                        eps: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``euclid_project`` on the tile kernel (rayen_proj_tile.hip)."""
    return proj_forward_raw(q, _pack(pack_id), max_iters, eps, kernel="tile")


@euclid_project_tile.register_fake
def _(q, pack_id, max_iters, eps):
    pack = _pack(pack_id)
    B = q.shape[0]
    return q.new_empty((B, pack.n)), q.new_empty((B,), dtype=torch.int32), q.new_empty((B, pack.m))


@torch.library.custom_op("rayen_amd::euclid_project_tile_bwd", mutates_args=())
def euclid_project_tile_bwd(grad_z: torch.Tensor, vstar: torch.Tensor, iters: torch.Tensor, pack_id: int, max_iters: int,
                            eps: float) -> torch.Tensor:
    return proj_backward_raw(grad_z, vstar, iters, _pack(pack_id), max_iters, eps, kernel="tile")


@euclid_project_tile_bwd.register_fake
def _(grad_z, vstar, iters, pack_id, max_iters, eps):
    return grad_z.new_empty((grad_z.shape[0], _pack(pack_id).n))


def _proj_tile_backward(ctx, grad_z, grad_iters, grad_vstar):
    vstar, iters = ctx.saved_tensors
    if grad_z is None:
        return None, None, None, None
    pack = _pack(ctx.pack_id)
    grad_q = torch.ops.rayen_amd.euclid_project_tile_bwd(grad_z.to(vstar.dtype), vstar, iters, ctx.pack_id, ctx.max_iters,
                                                         ctx.eps)
    if ctx.width > pack.n:          # columns of q beyond n are not read
        grad_q = torch.nn.functional.pad(grad_q, (0, ctx.width - pack.n))
    return grad_q, None, None, None


euclid_project_tile.register_autograd(_proj_tile_backward, setup_context=_proj_setup_context)


def proj_tile64_served(pack):
    """Does the fp64 tile kernel serve this pack's program (its envelope: ``served()`` in rayen_proj_tile64_layout.h)?
    Uploads the fp64 tile images on first use (an allocation and a copy: not while a stream is capturing)."""
    pack.tile64_images()
    return bool(_entry("rayen_proj_tile64_served")(pack.handle))


@torch.library.custom_op("rayen_amd::euclid_project_tile64", mutates_args=())
def euclid_project_tile64(q: torch.Tensor, pack_id: int, max_iters: int,
                          eps: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``euclid_project`` in fp64 on the fp64 tile kernel (rayen_proj_tile64.hip)."""
    return proj_forward_raw(q, _pack(pack_id), max_iters, eps, kernel="tile64")


@euclid_project_tile64.register_fake
def _(q, pack_id, max_iters, eps):
    pack = _pack(pack_id)
    B = q.shape[0]
    return q.new_empty((B, pack.n)), q.new_empty((B,), dtype=torch.int32), q.new_empty((B, pack.m))


@torch.library.custom_op("rayen_amd::euclid_project_tile64_bwd", mutates_args=())
def euclid_project_tile64_bwd(grad_z: torch.Tensor, vstar: torch.Tensor, iters: torch.Tensor, pack_id: int, max_iters: int,
                              eps: float) -> torch.Tensor:
    return proj_backward_raw(grad_z, vstar, iters, _pack(pack_id), max_iters, eps, kernel="tile64")


@euclid_project_tile64_bwd.register_fake
def _(grad_z, vstar, iters, pack_id, max_iters, eps):
    return grad_z.new_empty((grad_z.shape[0], _pack(pack_id).n))


def _proj_tile64_backward(ctx, grad_z, grad_iters, grad_vstar):
    vstar, iters = ctx.saved_tensors
    if grad_z is None:
        return None, None, None, None
    pack = _pack(ctx.pack_id)
    grad_q = torch.ops.rayen_amd.euclid_project_tile64_bwd(grad_z.to(vstar.dtype), vstar, iters, ctx.pack_id, ctx.max_iters,
                                                           ctx.eps)
    if ctx.width > pack.n:          # columns of q beyond n are not read
        grad_q = torch.nn.functional.pad(grad_q, (0, ctx.width - pack.n))
    return grad_q, None, None, None


euclid_project_tile64.register_autograd(_proj_tile64_backward, setup_context=_proj_setup_context)


# ------------------------------------------------------------------------------------------------
# soft cost and violation (examples/cost_computer.py:69-110, ConvexConstraints.getResiduals): loss + gradient on rayen_cost.hip
# and, for a set's LMI, rayen_cost_lmi.hip
# ------------------------------------------------------------------------------------------------

class CostPack(_SidePack):
    """Owner of one ``RayenCostPack*``: fp32 and fp64 images of a set's stacked rows (``soft_cost.set_arrays``) and of its
    LMI's generators, when it has one, on one device."""
    _layer = "cost"

    def __init__(self, arrays, device_index):
        a, ptr = arrays, _host_ptr
        self.k = int(a["k"])
        self._create(device_index, ptr(a["A1"]), ptr(a["b1"]), int(a["b1"].size), ptr(a["P"]), ptr(a["q"]), ptr(a["r"]),
                     int(a["r"].size), ptr(a["M"]), ptr(a["s"]), ptr(a["c"]), ptr(a["d"]), ptr(a["soc_rows"]),
                     int(a["soc_rows"].size), ptr(a["A2"]), ptr(a["b2"]), int(a["b2"].size), self.k)
        if a["F"].size:          # the set's LMI: F [k + 1, r, r] (rayen_cost_lmi.hip)
            with torch.cuda.device(self.device_index):
                _lib.check(_entry("rayen_cost_pack_set_lmi")(self.handle, ptr(a["F"]), int(a["F"].shape[-1])),
                           "rayen_cost_pack_set_lmi")

    def served(self, dtype):
        return bool(_entry("rayen_cost_served")(self.handle, int(dtype == torch.float64)))

    def stream_served(self, dtype, window_bytes=0):
        """Does the streamed route (``rayen_cost_stream.hip``: the stacked rows through LDS in windows of ``window_bytes``
        bytes, 0 = the default of 80 KiB) serve the set at ``dtype``?  The first call, and every call with another window
        size, builds and uploads the stream images; a pack nobody asks holds none."""
        with torch.cuda.device(self.device_index):
            _lib.check(_entry("rayen_cost_stream_set")(self.handle, int(window_bytes)), "rayen_cost_stream_set")
        self._stream_set = True
        return bool(_entry("rayen_cost_stream_served")(self.handle, int(dtype == torch.float64)))

    def tile64_served(self, window_bytes=0):
        """Does the fp64 tile route (``rayen_cost_tile64.hip``: blocks of 16 stacked rows on the fp64 matrix cores, the image
        through LDS in windows of ``window_bytes`` bytes, 0 = the default of 80 KiB) serve the set?  The first call, and every
        call with another window size, builds and uploads the image; a pack nobody asks holds none."""
        with torch.cuda.device(self.device_index):
            _lib.check(_entry("rayen_cost_tile64_set")(self.handle, int(window_bytes)), "rayen_cost_tile64_set")
        self._tile64_set = True
        return bool(_entry("rayen_cost_tile64_served")(self.handle))


COST_KERNELS = ("resident", "stream", "tile64")


def soft_cost_raw(y, pack, want_grad, kernel="resident"):
    """``(cost [B], worst [B], which [B] int32, grad [B, k] | None)`` of ``y [B, >= k]`` through ``rayen_soft_cost_*``
    (``kernel='resident'``: the image of the stacked rows in LDS) or ``rayen_soft_cost_stream_*`` (``'stream'``: the image
    through LDS in windows, at the window size of the pack's last ``stream_served`` call, the default if there was none) or
    ``rayen_soft_cost_tile64_f64`` (``'tile64'``: blocks of 16 rows on the fp64 matrix cores, at the window size of the pack's
    last ``tile64_served`` call; fp64 only: an fp32 call is refused with ``E_UNSUPPORTED``): one launch (two for a set that has
    an LMI next to other constraints)."""
    if kernel not in COST_KERNELS:
        raise ValueError(f"rayen_amd: kernel must be one of {COST_KERNELS}, got {kernel!r}")
    _check_rows(y, pack.k, pack, "y", "cost")
    name = "rayen_soft_cost"
    if kernel == "stream":
        name = "rayen_soft_cost_stream"
        if not getattr(pack, "_stream_set", False):
            with torch.cuda.device(pack.device_index):
                _lib.check(_entry("rayen_cost_stream_set")(pack.handle, 0), "rayen_cost_stream_set")
            pack._stream_set = True
    entry = None
    if kernel == "tile64":
        name = "rayen_soft_cost_tile64"
        if y.dtype != torch.float64:
            raise _lib.RayenError(_lib.E_UNSUPPORTED, name)
        if not getattr(pack, "_tile64_set", False):
            pack.tile64_served()
        entry = _entry("rayen_soft_cost_tile64_f64")
    y = _dense_rows(y, pack.k)
    B = y.shape[0]
    cost = torch.empty((B,), dtype=y.dtype, device=y.device)
    worst = torch.empty((B,), dtype=y.dtype, device=y.device)
    which = torch.empty((B,), dtype=torch.int32, device=y.device)
    grad = torch.empty((B, pack.k), dtype=y.dtype, device=y.device) if want_grad else None
    with _on_device(y.device):
        code = (entry or _typed(name, y.dtype))(
            pack.handle, _ptr(y), B, y.stride(0) if B else pack.k, _ptr(cost), _ptr(worst), _ptr(which), _ptr(grad),
            pack.k, _stream(y.device.index))
    _lib.check(code, name)
    return cost, worst, which, grad


@torch.library.custom_op("rayen_amd::soft_cost", mutates_args=())
def soft_cost(y: torch.Tensor, pack_id: int, need_grad: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(cost [B], worst [B], which [B] int32, grad [B, k])``; ``grad`` (``d cost[b] / d y[b]``, computed by the same
    launch) is empty (``[0, k]``) unless ``need_grad``."""
    pack = _pack(pack_id)
    cost, worst, which, grad = soft_cost_raw(y, pack, need_grad)
    return cost, worst, which, (grad if grad is not None else y.new_empty((0, pack.k)))


@soft_cost.register_fake
def _(y, pack_id, need_grad):
    B, k = y.shape[0], _pack(pack_id).k
    return (y.new_empty((B,)), y.new_empty((B,)), y.new_empty((B,), dtype=torch.int32),
            y.new_empty((B if need_grad else 0, k)))


def _cost_setup_context(ctx, inputs, output):
    y, _, need_grad = inputs
    ctx.width, ctx.have_grad = y.shape[1], bool(need_grad)
    ctx.save_for_backward(output[3])


def _cost_backward(ctx, grad_cost, grad_worst, grad_which, grad_grad):
    (grad,) = ctx.saved_tensors
    if grad_cost is None:
        return None, None, None
    if not ctx.have_grad:
        raise RuntimeError("rayen_amd::soft_cost was called with need_grad=False; its gradient was not computed")
    out = grad_cost.to(grad.dtype)[:, None] * grad
    if ctx.width > grad.shape[1]:          # columns of y beyond k are not read
        out = torch.nn.functional.pad(out, (0, ctx.width - grad.shape[1]))
    return out, None, None


soft_cost.register_autograd(_cost_backward, setup_context=_cost_setup_context)


@torch.library.custom_op("rayen_amd::soft_cost_stream", mutates_args=())
def soft_cost_stream(y: torch.Tensor, pack_id: int, need_grad: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``rayen_amd::soft_cost`` on the streamed route (``rayen_cost_stream.hip``): the same outputs, bit for bit where both
    serve the set, and the same autograd."""
    pack = _pack(pack_id)
    cost, worst, which, grad = soft_cost_raw(y, pack, need_grad, kernel="stream")
    return cost, worst, which, (grad if grad is not None else y.new_empty((0, pack.k)))


@soft_cost_stream.register_fake
def _(y, pack_id, need_grad):
    B, k = y.shape[0], _pack(pack_id).k
    return (y.new_empty((B,)), y.new_empty((B,)), y.new_empty((B,), dtype=torch.int32),
            y.new_empty((B if need_grad else 0, k)))


soft_cost_stream.register_autograd(_cost_backward, setup_context=_cost_setup_context)


@torch.library.custom_op("rayen_amd::soft_cost_tile64", mutates_args=())
def soft_cost_tile64(y: torch.Tensor, pack_id: int, need_grad: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``rayen_amd::soft_cost`` on the fp64 tile route (``rayen_cost_tile64.hip``): the same outputs (against the lane
    kernels the differences are summation order) and the same autograd; fp64 rows only."""
    pack = _pack(pack_id)
    cost, worst, which, grad = soft_cost_raw(y, pack, need_grad, kernel="tile64")
    return cost, worst, which, (grad if grad is not None else y.new_empty((0, pack.k)))


@soft_cost_tile64.register_fake
def _(y, pack_id, need_grad):
    B, k = y.shape[0], _pack(pack_id).k
    return (y.new_empty((B,)), y.new_empty((B,)), y.new_empty((B,), dtype=torch.int32),
            y.new_empty((B if need_grad else 0, k)))


soft_cost_tile64.register_autograd(_cost_backward, setup_context=_cost_setup_context)
