"""The module's mapper fused into the fp64 matrix-core forward (``fuse_mapper64=True``, ``rayen_amd::ray_project_mapped64``,
include/rayen_hip_mapped64.h) on an MI355X: ``ConstraintModule(cs, input_dim=..., create_map=True).double()`` =
rayen/constraint_module.py:259-263 + :525 + :468-474 in one launch.  Checked against the fp64 oracle fed with
``v = x W' + b`` formed on the host, against the two-op path, against ``np.longdouble`` for ``v`` itself, and bit for bit
against the unfused kernel on the ``v`` the fused call wrote."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import csd_from_cs, kink_mask, load_golden, rel_err_rows
from oracle import rayen_oracle as oracle
from rayen_amd import _lib, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

pytestmark = pytest.mark.gpu

FP64_TOL = 1e-9      # of a row, as tests/test_gpu_parity.py: two fp64 evaluations that differ by summation order
DEV = torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _sets():                                                  # as tests/test_gpu_mapper.py::_sets
    mixed_raw, _, _ = load_golden("example_13")
    return {
        "c1": workloads.make_raw("c1"),
        "c2": workloads.make_raw("c2", seed=41),
        "c3": workloads.make_raw("c3", seed=42),
        "c5r": workloads.make_raw("c5r", seed=43),
        "wide": workloads.random_lin_quad_soc(k=96, m=160, n_quad=2, n_soc=1, seed=44),
        "eq60": workloads.corridor_like(k=60, n_eq=10, m=120, n_quad=12, rank=3, seed=45),
        "ex13": mixed_raw,
    }


@functools.lru_cache(maxsize=None)
def _cs(name):
    return workloads.build_constraints(_sets()[name])


def _module(name, d, bias=True):
    """The module under the fp64 default dtype, as the reference trains (examples/main.py:288) and as
    tests/test_gpu_parity.py::_layer builds its fp64 layers: built under the fp32 default the set's constants are rounded
    to fp32 before ``.double()`` widens them, and no fp64 oracle is met to 1e-9 (2e-8 on c3, on either route)."""
    cs = _cs(name)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(0)
        layer = ConstraintModule(cs, input_dim=d, create_map=True, fuse_mapper64=True)
        if not bias:
            layer.mapper = torch.nn.Linear(d, cs.n, bias=False)
        return cs, layer.double().cuda()
    finally:
        torch.set_default_dtype(prev)


def _x(B, d, seed=5):
    x = torch.empty(B, d, dtype=torch.float64).uniform_(-2.0, 2.0, generator=torch.Generator().manual_seed(seed))
    x[:4] *= 1e-4
    return x


def _host_v(layer, x):
    w = layer.mapper.weight.detach().cpu().double()
    b = layer.mapper.bias.detach().cpu().double() if layer.mapper.bias is not None else 0.0
    return x.cpu().double() @ w.T + b


@functools.lru_cache(maxsize=None)
def _oracle_buf(name):
    return oracle.precompute(csd_from_cs(_cs(name)), torch.float64)


def _oracle_y(name, layer, x):
    return oracle.forward(_oracle_buf(name), _host_v(layer, x).unsqueeze(2)).numpy()[:, :, 0]


def _fused(layer, x, need_grad=False):
    _, pack_id = layer.device_pack(DEV)
    with torch.no_grad():
        return torch.ops.rayen_amd.ray_project_mapped64(x, layer.mapper.weight, layer.mapper.bias, pack_id, need_grad)


def _two_op(layer, x):
    layer.fuse_mapper64 = False
    try:
        with torch.no_grad():
            return layer(x)[:, :, 0]
    finally:
        layer.fuse_mapper64 = True


# ------------------------------------------------------------------------------------------------ 1. forward

_FORWARD = ([("c3", d, B, True) for d in (1, 4, 31, 32, 33, 65, 100, 512) for B in (1000,)]
            + [(name, 64, B, True) for name in ("c3", "c5r") for B in (1, 31, 33, 1000)]
            + [("c3", 513, 1000, False), ("c2", 8, 1000, True), ("c2", 64, 1000, True), ("c5r", 32, 1000, True),
               ("eq60", 40, 1000, True), ("c1", 8, 1000, False), ("ex13", 8, 1000, False), ("wide", 48, 1000, False)])


@pytest.mark.parametrize("name,d,B,fusable", _FORWARD)
def test_fused_forward_matches_oracle_and_two_op_path(name, d, B, fusable):
    cs, layer = _module(name, d)
    x = _x(B, d)
    xd = x.cuda()
    dp, _ = layer.device_pack(DEV)
    assert ops.mapper_fusable64(xd, layer.mapper.weight, layer.mapper.bias, dp) == fusable
    assert dp.mapper_mode64(d) == int(fusable)
    if not fusable:
        with pytest.raises(RuntimeError, match="unsupported mapper"):
            _fused(layer, xd)
        with torch.no_grad():
            y = layer(xd)                                    # the two-op path, silently
        assert torch.equal(y[:, :, 0], _two_op(layer, xd))
        return
    with torch.no_grad():
        y_fused = layer(xd)
    assert _lib.load().rayen_last_forward_kernel() == _lib.KERNEL_MFMA
    assert y_fused.shape == (B, cs.k, 1) and y_fused.dtype == torch.float64
    assert torch.equal(y_fused[:, :, 0], _fused(layer, xd)[0])          # the module went through the fused op
    y_fused = y_fused.cpu().numpy()[:, :, 0]
    y_ref = _oracle_y(name, layer, x)
    y_two = _two_op(layer, xd).cpu().numpy()
    err_ref, err_two = rel_err_rows(y_fused, y_ref).max(), rel_err_rows(y_fused, y_two).max()
    print(f"{name}/{d} B={B}: fused vs oracle {err_ref:.3e}, vs two-op {err_two:.3e}")
    assert err_ref < FP64_TOL and err_two < FP64_TOL


def test_empty_batch_returns_empty_tensors():
    cs, layer = _module("c3", 64)
    xd = torch.empty(0, 64, dtype=torch.float64, device=DEV)
    for need_grad in (False, True):
        y, kappa, active, v = _fused(layer, xd, need_grad)
        assert y.shape == (0, cs.k) and kappa.shape == (0,) and active.shape == (0, 2) and v.shape == (0, cs.n)
    with torch.no_grad():
        assert layer(xd).shape == (0, cs.k, 1)


# ------------------------------------------------------------------------------------------------ 2. v itself

def _v_bound(layer, x):
    """(exact v in long double, the forward error bound of ANY summation order of in_dim + 1 terms with FMAs)."""
    w = layer.mapper.weight.detach().cpu().numpy().astype(np.longdouble)
    xl = x.cpu().numpy().astype(np.longdouble)
    exact, mag = xl @ w.T, np.abs(xl) @ np.abs(w).T
    if layer.mapper.bias is not None:
        b = layer.mapper.bias.detach().cpu().numpy().astype(np.longdouble)
        exact, mag = exact + b, mag + np.abs(b)
    return exact, (x.shape[1] + 2) * np.longdouble(2.0) ** -53 * mag


@pytest.mark.parametrize("name,d", [("c3", 64), ("c3", 33), ("c3", 512), ("c2", 8), ("c5r", 64), ("eq60", 40)])
def test_v_is_the_linear_map_to_the_derived_bound(name, d):
    cs, layer = _module(name, d)
    x = _x(1000, d, seed=7)
    _, _, active, v = _fused(layer, x.cuda(), need_grad=True)
    assert v.shape == (1000, cs.n) and active.shape == (1000, 2)
    exact, bound = _v_bound(layer, x)
    err = np.abs(v.cpu().numpy().astype(np.longdouble) - exact)
    print(f"{name}/{d}: worst |v - exact| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("name,d", [("c3", 64), ("c5r", 64), ("c2", 8)])
def test_columns_of_v_beyond_n_are_never_written(name, d):
    cs, layer = _module(name, d)
    dp, _ = layer.device_pack(DEV)
    B, ldvo = 77, cs.n + 7
    x = _x(B, d, seed=9).cuda()
    v_wide = torch.full((B + 1, ldvo), -7.25, dtype=torch.float64, device=DEV)     # (one spare row past the batch)
    y = torch.empty(B, cs.k, dtype=torch.float64, device=DEV)
    kappa = torch.empty(B, dtype=torch.float64, device=DEV)
    active = torch.empty(B, 2, dtype=torch.int32, device=DEV)
    w, b = layer.mapper.weight.detach(), layer.mapper.bias.detach()
    code = _lib.load().rayen_ray_project_mapped_f64(
        dp.handle, x.data_ptr(), B, d, d, w.data_ptr(), w.stride(0), b.data_ptr(), v_wide.data_ptr(), ldvo,
        y.data_ptr(), cs.k, kappa.data_ptr(), active.data_ptr(), dp.nan_flag.data_ptr(),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert code == 0
    assert torch.all(v_wide[:B, cs.n:] == -7.25) and torch.all(v_wide[B] == -7.25)
    y2, kappa2, active2, v2 = _fused(layer, x, need_grad=True)
    assert torch.equal(v_wide[:B, :cs.n], v2) and torch.equal(y, y2) and torch.equal(kappa, kappa2) and torch.equal(active, active2)


# ------------------------------------------------------------------------------------------------ 3. same walk, same bits

@pytest.mark.parametrize("name,d", [("c3", 64), ("c5r", 64), ("eq60", 40)])
def test_the_walk_behind_the_mapper_is_the_unfused_walk_bit_for_bit(name, d):
    cs, layer = _module(name, d)
    dp, _ = layer.device_pack(DEV)
    x = _x(1000, d, seed=12).cuda()
    y, kappa, active, v = _fused(layer, x, need_grad=True)
    y_raw, kappa_raw, active_raw = ops.project_raw(v, dp)
    assert torch.equal(y, y_raw) and torch.equal(kappa, kappa_raw) and torch.equal(active, active_raw)
    y0, kappa0, active0, v0 = _fused(layer, x, need_grad=False)
    assert torch.equal(y0, y) and torch.equal(kappa0, kappa) and v0.numel() == 0 and active0.numel() == 0


# ------------------------------------------------------------------------------------------------ 4. row independence

@pytest.mark.parametrize("name", ["c3", "c5r"])
def test_rows_do_not_depend_on_their_neighbours(name):
    cs, layer = _module(name, 64)
    big = _x(70, 64, seed=13).cuda()
    x = big[5:38].contiguous()                                # 33 rows
    y, kappa, active, v = _fused(layer, x, need_grad=True)
    yb, kb, ab, vb = _fused(layer, big, need_grad=True)
    assert torch.equal(yb[5:38], y) and torch.equal(kb[5:38], kappa) and torch.equal(ab[5:38], active) and torch.equal(vb[5:38], v)
    for i in range(33):
        y1, k1, a1, v1 = _fused(layer, x[i:i + 1], need_grad=True)
        assert torch.equal(y1[0], y[i]) and torch.equal(k1[0], kappa[i]) and torch.equal(a1[0], active[i]) and torch.equal(v1[0], v[i])
    # a NaN row stays in its row, and the module says so
    xn = x.clone()
    xn[17] = float("nan")
    yn = _fused(layer, xn)[0]
    keep = [i for i in range(33) if i != 17]
    assert torch.equal(yn[keep], y[keep]) and torch.isnan(yn[17]).any()
    dp, _ = layer.device_pack(DEV)
    dp.nan_flag.zero_()
    with pytest.raises(AssertionError, match="NaN"):
        with torch.no_grad():
            layer(xn)
    with torch.no_grad():
        assert torch.equal(layer(x)[:, :, 0], y)                # (the flag was cleared)


# ------------------------------------------------------------------------------------------------ 5. strides and bias

def test_strided_input_strided_weight_and_no_bias():
    cs, layer = _module("c3", 64)
    big = torch.empty(777, 69, dtype=torch.float64).uniform_(-1.5, 1.5, generator=torch.Generator().manual_seed(6))
    x = big[:, :64]                                           # ldx = in_dim + 5
    xd = big.cuda()[:, :64]
    dp, pack_id = layer.device_pack(DEV)
    assert xd.stride(0) == 69 and ops.mapper_fusable64(xd, layer.mapper.weight, layer.mapper.bias, dp)
    with torch.no_grad():
        y = layer(xd)[:, :, 0]
    assert torch.equal(y, _fused(layer, xd.contiguous())[0])
    assert rel_err_rows(y.cpu().numpy(), _oracle_y("c3", layer, x)).max() < FP64_TOL
    # weight as a column slice of a wider matrix (ldw > in_dim), odd offsets: only 8-byte alignment
    w_big = torch.zeros(cs.n, 71, dtype=torch.float64, device=DEV)
    w_big[:, 3:67] = layer.mapper.weight.detach()
    w_view = w_big[:, 3:67]
    assert w_view.stride(0) == 71 and ops.mapper_fusable64(xd, w_view, layer.mapper.bias, dp)
    with torch.no_grad():
        out = torch.ops.rayen_amd.ray_project_mapped64(xd, w_view, layer.mapper.bias, pack_id, True)
    ref = _fused(layer, xd, need_grad=True)
    assert all(torch.equal(a, b) for a, b in zip(out, ref))
    w_gaps = torch.zeros(cs.n, 128, dtype=torch.float64, device=DEV)[:, ::2]                    # column stride 2
    assert w_gaps.shape == w_view.shape and not ops.mapper_fusable64(xd, w_gaps, layer.mapper.bias, dp)
    # bias=False
    for name, d in (("c3", 32), ("c5r", 64)):
        cs2, nb = _module(name, d, bias=False)
        assert nb.mapper.bias is None
        x2 = _x(500, d, seed=14)
        with torch.no_grad():
            y2 = nb(x2.cuda())[:, :, 0]
        assert torch.equal(y2, _fused(nb, x2.cuda())[0])
        assert rel_err_rows(y2.cpu().numpy(), _oracle_y(name, nb, x2)).max() < FP64_TOL


def test_weight_updates_reach_the_fused_kernel_at_once():
    cs, layer = _module("c3", 64)
    x = _x(500, 64, seed=11)
    with torch.no_grad():
        y_a = layer(x.cuda()).clone()
        layer.mapper.weight.mul_(0.5)
        layer.mapper.bias.add_(0.25)
        y_b = layer(x.cuda()).clone()
    assert not torch.equal(y_a, y_b)
    assert rel_err_rows(y_b.cpu().numpy()[:, :, 0], _oracle_y("c3", layer, x)).max() < FP64_TOL
    layer.mapper.weight.data.mul_(1.5)                        # behind the version counter
    for prm in layer.mapper.parameters():
        prm.requires_grad_(False)                             # (frozen: nothing is cached for them either)
    with torch.no_grad():
        y_c = layer(x.cuda()).clone()
        layer.mapper.weight.data.mul_(0.5)
        y_d = layer(x.cuda()).clone()
    assert not torch.equal(y_c, y_b) and not torch.equal(y_d, y_c)
    assert rel_err_rows(y_d.cpu().numpy()[:, :, 0], _oracle_y("c3", layer, x)).max() < FP64_TOL


# ------------------------------------------------------------------------------------------------ 6. gradients

@pytest.mark.parametrize("name,d", [("c2", 8), ("c2", 64), ("c3", 64), ("c3", 36), ("c5r", 32), ("c5r", 64), ("eq60", 40)])
def test_gradients_of_the_fused_layer_match_the_two_op_path(name, d):
    cs, layer = _module(name, d)
    gen = torch.Generator().manual_seed(8)
    x = torch.empty(640, d, dtype=torch.float64).uniform_(-2.0, 2.0, generator=gen)
    G = torch.empty(640, cs.k, 1, dtype=torch.float64).uniform_(-1.0, 1.0, generator=gen).cuda()
    # no row sits on a kink of the layer (checked on the fp64 oracle): every row is compared
    v_host = _host_v(layer, x).unsqueeze(2)
    assert int(kink_mask(oracle, cs, v_host, 1e-9).sum()) == 0
    dp, _ = layer.device_pack(DEV)
    active_fused = _fused(layer, x.cuda(), need_grad=True)[2]
    with torch.no_grad():
        v_two = torch.nn.functional.linear(x.cuda(), layer.mapper.weight, layer.mapper.bias)
    active_two = ops.project_raw(v_two, dp)[2]
    assert torch.equal(active_fused, active_two)

    def grads(fuse):
        layer.fuse_mapper64 = fuse
        layer.zero_grad()
        xg = x.cuda().requires_grad_(True)
        (layer(xg) * G).sum().backward()
        return xg.grad.cpu(), layer.mapper.weight.grad.cpu().clone(), layer.mapper.bias.grad.cpu().clone()

    fused, two_op = grads(True), grads(False)
    layer.fuse_mapper64 = True
    for what, a, b in zip(("grad_x", "grad_weight", "grad_bias"), fused, two_op):
        worst = float((a - b).abs().max()) / float(b.abs().max())
        print(f"{name}/{d} {what}: {worst:.3e} of the largest entry")
        assert worst < FP64_TOL, what


# ------------------------------------------------------------------------------------------------ 7. capture, 8. opcheck

def test_fused_layer_under_hip_graph_capture():
    cs, layer = _module("c3", 64)
    layer.check_nan = False
    x = torch.randn(2048, 64, device="cuda", dtype=torch.float64)
    with torch.no_grad():
        eager = layer(x).clone()
        assert _lib.load().rayen_last_forward_kernel() == _lib.KERNEL_MFMA
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            layer(x)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = layer(x)
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_opcheck_ray_project_mapped64():
    cs, layer = _module("c3", 32)
    _, pack_id = layer.device_pack(DEV)
    x = torch.randn(130, 32, device="cuda", dtype=torch.float64, requires_grad=True)
    torch.library.opcheck(torch.ops.rayen_amd.ray_project_mapped64.default,
                          (x, layer.mapper.weight, layer.mapper.bias, pack_id, True),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
