"""What the Python wrappers of the four side layers (``method='Bar'``, ``method='DC3'``, the Euclidean projection, the soft
cost; ``rayen_amd/ops.py``) promise around their kernels, whichever precision: which inputs they refuse and in what words,
an empty batch, rows with a stride of their own, the scratch sizes the library reports, and packs that have been closed.

The packs are the smallest the other modules build (Bar: ``k = 5, nv = 9, nr = 4`` of ``test_gpu_ops.py``; the first case of
``dc3_reference``, ``proj_reference`` and ``cost_cases``) and the batches three rows: the subject is the plumbing, not the
arithmetic, and nothing here is compared with a reference other than the same call on a contiguous copy (bit for bit).

A raw call on a closed pack: Bar and the soft cost reach the entry point, which answers ``RAYEN_E_BAD_ARG``
(``_lib.RayenError``).  DC3 and the projection size a scratch buffer before they reach it, and the call is refused there, as
a ``RuntimeError`` naming ``rayen_*_workspace_bytes``; for these two the module pins that, not ``_lib.RayenError``."""
import functools
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from rayen_amd import _lib, ops

import cost_cases
import cost_sweep_cases
import dc3_reference
import proj_reference
import side_layout_formulas as formulas

pytestmark = pytest.mark.gpu

LAYERS = ("bar", "dc3", "proj", "cost")
DTYPES = (torch.float32, torch.float64)
DC3_CASE = dc3_reference.CASES[0]
DC3_STEPS = 33               # two chunks of steps: the states between launches are in use; eps = 0 runs them all
PROJ_CASE = proj_reference.CASES[0].name
PROJ_ITERS, PROJ_EPS = 64, 1e-6


def _bar():
    rng = np.random.default_rng(9)
    return ops.BarPack(rng.normal(size=(5, 13)), rng.normal(size=5), 9, 4, 0)


def _layer(name):
    """width: columns the layer reads | what: its name for the input | noun: its name for itself | raw / op: the forward
    through the raw wrapper and through the custom op (the op's first output is differentiable) | shapes: of raw's outputs."""
    if name == "bar":
        return SimpleNamespace(
            make=_bar, width=lambda p: p.width, what="q", noun="the Bar layer's HIP op",
            raw=lambda q, p: ops.bar_forward_raw(q, p),
            op=lambda q, pid: torch.ops.rayen_amd.bar_project(q, pid),
            shapes=lambda B, p: [(B, p.k), (B,)], closed=_lib.RayenError, closed_match="rayen_bar_forward")
    if name == "dc3":
        args = (DC3_CASE.lr, dc3_reference.MOMENTUM, 0.0, DC3_STEPS)
        return SimpleNamespace(
            make=lambda: ops.Dc3Pack(dc3_reference.make_pack(DC3_CASE), 0), width=lambda p: p.n, what="q",
            noun="the DC3 layer's HIP op",
            raw=lambda q, p: ops.dc3_forward_raw(q, p, *args),
            op=lambda q, pid: torch.ops.rayen_amd.dc3_project(q, pid, *args),
            shapes=lambda B, p: [(B, p.k), (1,)], closed=RuntimeError,
            closed_match="rayen_dc3_workspace_bytes refused its arguments")
    if name == "proj":
        return SimpleNamespace(
            make=lambda: ops.ProjPack(proj_reference.module_for(PROJ_CASE).program.arrays(), 0), width=lambda p: p.n,
            what="q", noun="the projection's HIP op",
            raw=lambda q, p: ops.proj_forward_raw(q, p, PROJ_ITERS, PROJ_EPS),
            op=lambda q, pid: torch.ops.rayen_amd.euclid_project(q, pid, PROJ_ITERS, PROJ_EPS),
            shapes=lambda B, p: [(B, p.n), (B,), (B, p.m)], closed=RuntimeError,
            closed_match="rayen_proj_workspace_bytes refused its arguments")
    return SimpleNamespace(
        make=lambda: ops.CostPack(cost_cases.case(cost_cases.NAMES[0]).arrays, 0), width=lambda p: p.k, what="y",
        noun="the soft-cost HIP op",
        raw=lambda q, p: ops.soft_cost_raw(q, p, True),
        op=lambda q, pid: torch.ops.rayen_amd.soft_cost(q, pid, True),
        shapes=lambda B, p: [(B,), (B,), (B,), (B, p.k)], closed=_lib.RayenError, closed_match="rayen_soft_cost")


@functools.lru_cache(maxsize=None)
def _live(name):
    """(layer, its pack, the pack's id): built once, never closed"""
    layer = _layer(name)
    pack = layer.make()
    return layer, pack, ops.register_pack(pack)


def _rows(B, cols, dtype, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + 10 * B + cols)
    return (1.5 * torch.randn(B, cols, generator=gen, dtype=torch.float64)).to(dtype)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _forward_and_gradient(layer, pack_id, q):
    """the op's outputs and the gradient of <its first output, fixed weights> with respect to ``q``"""
    q = q.detach().requires_grad_(True)
    out = layer.op(q, pack_id)
    weights = _rows(*out[0].shape, q.dtype, seed=1).cuda() if out[0].dim() == 2 else \
        _rows(out[0].shape[0], 1, q.dtype, seed=1).cuda()[:, 0]
    (grad,) = torch.autograd.grad(out[0], q, weights)
    return [t.detach() for t in out], grad


# ---- refused inputs

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", LAYERS)
def test_refused_inputs_name_the_layer_and_the_fault(name, dtype):
    layer, pack, _ = _live(name)
    w = layer.width(pack)
    good = _rows(3, w, dtype)
    with pytest.raises(RuntimeError, match=re.escape(f"rayen_amd: {layer.noun} runs on an MI355X (HIP) device only; got a "
                                                     "cpu tensor")):
        layer.raw(good, pack)
    with pytest.raises(RuntimeError, match=re.escape("rayen_amd: unsupported dtype torch.float16 (float32 and float64 "
                                                     "only)")):
        layer.raw(good.cuda().half(), pack)
    with pytest.raises(RuntimeError, match=re.escape(f"rayen_amd: expected {layer.what} of shape [B, >= {w}], got "
                                                     f"({w},)")):
        layer.raw(good.cuda()[0], pack)
    with pytest.raises(RuntimeError, match=re.escape(f"rayen_amd: expected {layer.what} of shape [B, >= {w}], got "
                                                     f"(3, {w - 1})")):
        layer.raw(_rows(3, w - 1, dtype).cuda(), pack)


@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_inputs_of_the_backward_wrappers(dtype):
    """the backward wrappers test their first argument the same way; the projection's is called ``grad_z``"""
    _, bar, _ = _live("bar")
    _, dc3, _ = _live("dc3")
    _, proj, _ = _live("proj")
    none = torch.empty(0, device="cuda")
    narrow = lambda p, w: _rows(3, w - 1, dtype).cuda()          # noqa: E731
    with pytest.raises(RuntimeError, match=re.escape(f"expected q of shape [B, >= {bar.width}], got (3, {bar.width - 1})")):
        ops.bar_backward_raw(narrow(bar, bar.width), none, none, bar)
    with pytest.raises(RuntimeError, match=re.escape(f"expected q of shape [B, >= {dc3.n}], got (3, {dc3.n - 1})")):
        ops.dc3_backward_raw(narrow(dc3, dc3.n), none, none, dc3, DC3_CASE.lr, dc3_reference.MOMENTUM, DC3_STEPS)
    with pytest.raises(RuntimeError, match=re.escape(f"expected grad_z of shape [B, >= {proj.n}], got (3, {proj.n - 1})")):
        ops.proj_backward_raw(narrow(proj, proj.n), none, none, proj, PROJ_ITERS, PROJ_EPS)
    with pytest.raises(RuntimeError, match=re.escape("the projection's HIP op runs on an MI355X (HIP) device only; got a cpu "
                                                     "tensor")):
        ops.proj_backward_raw(_rows(3, proj.n, dtype), none, none, proj, PROJ_ITERS, PROJ_EPS)


# ---- an empty batch

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", LAYERS)
def test_empty_batch_returns_the_documented_shapes(name, dtype):
    layer, pack, pack_id = _live(name)
    w = layer.width(pack)
    q = torch.empty(0, w, dtype=dtype, device="cuda")
    out = layer.raw(q, pack)
    assert [tuple(t.shape) for t in out] == layer.shapes(0, pack)
    assert out[0].dtype == dtype and out[0].is_cuda
    if name == "dc3":
        assert int(out[1]) == 0                  # an empty batch takes no step
    none = torch.empty(0, out[0].shape[1] if out[0].dim() == 2 else 0, dtype=dtype, device="cuda")
    if name == "bar":
        assert tuple(ops.bar_backward_raw(q, out[1], none, pack).shape) == (0, w)
    elif name == "dc3":
        grad = ops.dc3_backward_raw(q, out[1], none, pack, DC3_CASE.lr, dc3_reference.MOMENTUM, DC3_STEPS)
        assert tuple(grad.shape) == (0, w)
    elif name == "proj":
        assert tuple(ops.proj_backward_raw(none, out[2], out[1], pack, PROJ_ITERS, PROJ_EPS).shape) == (0, w)
    torch.cuda.synchronize()


# ---- rows with a stride of their own

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", LAYERS)
def test_strided_rows_answer_like_their_contiguous_copy(name, dtype):
    layer, pack, pack_id = _live(name)
    w = layer.width(pack)
    cols = w + 2
    stride = cols + 1 + (cols % 2)               # odd: the rows are neither contiguous nor 16-byte aligned (either precision)
    assert stride > cols and stride % 2 == 1 and (stride * q_bytes(dtype)) % 16 != 0
    buf = _rows(4, stride, dtype).cuda()
    view = buf.as_strided((3, cols), (stride, 1))
    assert not view.is_contiguous()
    dense = view.contiguous()
    raw_v, raw_d = layer.raw(view, pack), layer.raw(dense, pack)
    assert [tuple(t.shape) for t in raw_v] == layer.shapes(3, pack)
    assert all(_same(a, b) for a, b in zip(raw_v, raw_d))
    out_v, grad_v = _forward_and_gradient(layer, pack_id, view)
    out_d, grad_d = _forward_and_gradient(layer, pack_id, dense)
    assert all(_same(a, b) for a, b in zip(out_v, out_d))
    assert all(_same(a, b) for a, b in zip(out_v, raw_d))
    assert tuple(grad_v.shape) == (3, cols) and torch.equal(grad_v, grad_d)
    assert bool((grad_v[:, w:] == 0).all())
    assert bool(torch.isfinite(grad_v).all())
    if name != "proj":                           # (a row the projection moves onto a vertex has no gradient)
        assert bool((grad_v[:, :w] != 0).any())


def q_bytes(dtype):
    return 4 if dtype == torch.float32 else 8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", LAYERS)
def test_one_row_with_stride_zero(name, dtype):
    """one row whose stride addresses nothing and is below what the C ABI accepts (``_dense_rows``)"""
    layer, pack, pack_id = _live(name)
    w = layer.width(pack)
    view = _rows(1, w, dtype, seed=2).cuda().as_strided((1, w), (0, 1))
    assert view.stride() == (0, 1)
    dense = view.contiguous()
    raw_v, raw_d = layer.raw(view, pack), layer.raw(dense, pack)
    assert [tuple(t.shape) for t in raw_v] == layer.shapes(1, pack)
    assert all(_same(a, b) for a, b in zip(raw_v, raw_d))
    out_v, grad_v = _forward_and_gradient(layer, pack_id, view)
    out_d, grad_d = _forward_and_gradient(layer, pack_id, dense)
    assert all(_same(a, b) for a, b in zip(out_v, out_d))
    assert tuple(grad_v.shape) == (1, w) and torch.equal(grad_v, grad_d)


# ---- the scratch sizes the library reports

def test_workspace_bytes_are_the_written_out_formulas():
    lib = _lib.load()
    _, dc3, _ = _live("dc3")
    _, proj, _ = _live("proj")
    for B in formulas.BATCHES:
        for f64 in (0, 1):
            elem = 8 if f64 else 4
            for steps in formulas.STEPS:
                assert lib.rayen_dc3_workspace_bytes(dc3.handle, B, steps, f64, 0) == \
                    formulas.dc3_forward(dc3.n, B, steps, elem)[0], (B, steps, f64)
                assert lib.rayen_dc3_workspace_bytes(dc3.handle, B, steps, f64, 1) == \
                    formulas.dc3_backward(dc3.n, B, steps, elem)[0], (B, steps, f64)
            for backward in (0, 1):
                assert lib.rayen_proj_workspace_bytes(proj.handle, B, f64, backward) == \
                    formulas.proj(proj.n, proj.m, B, elem, backward)[0], (B, f64, backward)
    assert lib.rayen_dc3_workspace_bytes(None, 1, 1, 0, 0) == -1 and lib.rayen_dc3_workspace_bytes(dc3.handle, -1, 1, 0, 0) == -1
    assert lib.rayen_dc3_workspace_bytes(dc3.handle, 1, 0, 0, 0) == -1
    assert lib.rayen_proj_workspace_bytes(None, 1, 0, 0) == -1 and lib.rayen_proj_workspace_bytes(proj.handle, -1, 0, 0) == -1


# ---- closed packs

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", LAYERS)
def test_closed_packs(name, dtype):
    layer = _layer(name)
    pack = layer.make()
    pack_id = ops.register_pack(pack)
    assert ops._pack(pack_id) is pack
    q = _rows(3, layer.width(pack), dtype).cuda()
    layer.raw(q, pack)
    torch.cuda.synchronize()
    pack.close()
    pack.close()                                 # twice is harmless
    assert pack.handle is None
    with pytest.raises(layer.closed, match=layer.closed_match):
        layer.raw(q, pack)
    with pytest.raises(RuntimeError, match=f"constant pack {pack_id} no longer exists"):
        ops._pack(pack_id)
    del pack                                     # (its __del__ closes a third time)


# ---- soft cost: served

@pytest.mark.parametrize("dtype", DTYPES)
def test_k65_cost_pack_serves_neither_precision(dtype):
    pack = ops.CostPack(cost_sweep_cases.k65_case().arrays, torch.cuda.current_device())
    assert pack.k == 65 and pack.served(dtype) is False
    _, live, _ = _live("cost")
    assert live.served(dtype) is True
    pack.close()
