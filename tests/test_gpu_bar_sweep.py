"""Every instance of the Bar kernels (rayen_amd/csrc/rayen_bar.hip: forward / backward x fp32 / fp64 x K in
{4, 8, 16, 32, 64}, every lane-group width L) against the fp64 reference of tests/bar_reference.py, on synthetic packs
driven straight through ``ops.BarPack`` / ``ops.bar_forward_raw`` / ``ops.bar_backward_raw``.

The bar of the sweep is derived, not measured: in the scaled metric of bar_reference.py, ``C u`` with
``C = 4 ceil(pieces / L) + K + 48`` (bar_reference.tolerance_factor).  Each test prints the worst ``err / (C u)`` it saw.
Large logits are judged against the same formula evaluated by torch in the working precision (4 x its error, floor 16 u).
"""
import functools
import gc
import warnings

import numpy as np
import pytest
import torch

import bar_reference as br
from helpers import load_golden
from rayen_amd import _lib, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
_ids = {"ids": lambda v: v.name if isinstance(v, br.Case) else str(v).replace("torch.", "")}


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


@functools.lru_cache(maxsize=None)
def _pack(case):
    G, yp = br.make_pack(case)
    return ops.BarPack(G, yp, case.nv, case.nr, 0), _dev(G), _dev(yp)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _check(case, q, gy, what, tol_factor=None):
    """Forward and backward of ``q`` ([B, >= m], working precision, any layout the wrapper takes) against fp64.
    Returns the two errors over the tolerance."""
    bp, G, yp = _pack(case)
    k, nv, nr = case.k, case.nv, case.nr
    m = nv + nr
    u = br.U[q.dtype]
    tol = (tol_factor or br.tolerance_factor(case)) * u
    y, lse = ops.bar_forward_raw(q, bp)
    gq = ops.bar_backward_raw(q, lse, gy, bp)
    assert y.shape == (q.shape[0], k) and y.dtype == q.dtype and gq.shape == q.shape and gq.dtype == q.dtype
    q64, gy64 = q[:, :m].double(), gy.double()
    ef = br.scaled_err(y, br.forward64(G, yp, nv, nr, q64), br.forward_scale(G, yp, nv, nr, q64)).max().item()
    eb = br.scaled_err(gq[:, :m], br.backward64(G, nv, nr, q64, gy64), br.backward_scale(G, nv, nr, q64, gy64)).max().item()
    print(f"{case.name} {str(q.dtype)[6:]} K={br.pad_k(k)} L={br.lanes(m)} {what} B={q.shape[0]}: "
          f"forward {ef / tol:.3f} backward {eb / tol:.3f} of C u (C = {tol / u:.0f})")
    assert ef <= tol, (case.name, what, "forward", ef, tol)
    assert eb <= tol, (case.name, what, "backward", eb, tol)
    assert torch.isfinite(y).all() and torch.isfinite(gq[:, :m]).all()
    if nv:
        want = br.lse64(nv, q64)
        assert torch.all(torch.abs(lse.double() - want) <= 4 * u * (1 + want.abs())), (case.name, what, "rowstat")
    if q.shape[1] > m:
        assert torch.all(gq[:, m:] == 0)
    dead = torch.isinf(q64) | (q64 == 0)
    assert torch.all(gq[:, :m][dead] == 0)                     # exactly 0 on -inf logits and on zero ray entries
    if nv == 1:
        assert torch.all(gq[:, 0] == 0)                          # one vertex: weight 1, gradient 0, exactly
    return ef / tol, eb / tol


def _inputs(case, B, dtype, variant="plain", amplitude=5.0, width=None):
    q, gy = br.make_inputs(case, B, variant, amplitude, width)
    return _dev(q, dtype), _dev(gy, dtype)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("case", br.CASES, **_ids)
def test_sweep_small_batches(case, dtype):
    """B in {1, rows_per_iter - 1, rows_per_iter + 1}, plain logits and the -inf / zero variant."""
    worst = 0.0
    for B in br.sweep_batches(case):
        for variant in ("plain", "edges"):
            q, gy = _inputs(case, B, dtype, variant)
            worst = max(worst, *_check(case, q, gy, variant))
    print(f"worst err / (C u): {worst:.3f}")


BIG = ["L1_k4_mixed_piece_one_ray", "L2_k5_mixed_piece", "L4_k16_mixed_piece", "L8_k17_six_pieces", "L8_k32_rays_only",
       "L16_k33_ten_pieces", "L16_k64_simplex_like", "L16_k8_thousand_generators"]


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("name", BIG)
def test_sweep_second_trip_of_the_row_loop(name, dtype):
    """More rows than a full grid covers in one pass (multiProcessorCount * 4 workgroups of rows_per_iter rows)."""
    case = br.CASE[name]
    B = br.sweep_batches(case, _cus())[-1]
    assert B > _cus() * 4 * br.rows_per_iter(case.nv + case.nr)
    q, gy = _inputs(case, B, dtype, "edges")
    _check(case, q, gy, "second trip")


def test_empty_batch_and_k_beyond_64():
    case = br.CASE["L2_k5_mixed_piece"]
    bp, _, _ = _pack(case)
    for dtype in DTYPES:
        q = torch.empty(0, case.nv + case.nr, dtype=dtype, device=DEV)
        y, lse = ops.bar_forward_raw(q, bp)
        gq = ops.bar_backward_raw(q, lse, torch.empty(0, case.k, dtype=dtype, device=DEV), bp)
        assert y.shape == (0, case.k) and lse.shape == (0,) and gq.shape == q.shape
    with pytest.raises(_lib.RayenError) as err:
        ops.BarPack(np.ones((65, 4)), np.zeros(65), 4, 0, 0)
    assert err.value.code == _lib.E_UNSUPPORTED


LAYOUT_CASES = ["L2_k5_mixed_piece", "L4_k16_mixed_piece", "L16_k16_sixteen_pieces", "L16_k33_ten_pieces", "L16_k4_wide"]


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("layout", ["stride_m_plus_1", "base_off_by_one_element", "column_stride"])
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_sweep_layouts(name, layout, dtype):
    """(dense is every other test.)  Whatever lies beyond column m is NaN, so a read past m poisons y or grad_q."""
    case = br.CASE[name]
    m = case.nv + case.nr
    B = br.rows_per_iter(m) + 1
    q0, gy = _inputs(case, B, dtype, "edges")
    if layout == "stride_m_plus_1":
        q = torch.full((B, m + 1), float("nan"), dtype=dtype, device=DEV)
        q[:, :m] = q0
        assert q.stride(0) == m + 1
    elif layout == "base_off_by_one_element":
        ld = (m + 4) & ~3                                      # rows 16-byte multiples apart, the base is not aligned
        buf = torch.full((B * ld + 1,), float("nan"), dtype=dtype, device=DEV)
        q = buf[1:].view(B, ld)[:, :m]
        q.copy_(q0)
        assert (q.stride(0) * q.element_size()) % 16 == 0 and q.data_ptr() % 16 == q.element_size()
    else:
        q = torch.full((m + 3, B), float("nan"), dtype=dtype, device=DEV)
        q[:m] = q0.t()
        q = q.t()[:, :m]
        assert q.stride(1) != 1
    _check(case, q, gy, layout)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("off_q,off_g", [(0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("name", ["L4_k16_mixed_piece", "L16_k33_ten_pieces"])
def test_backward_with_differently_aligned_q_and_grad_q(name, off_q, off_g, dtype):
    """Straight through the C ABI: ``q`` and ``grad_q`` share ``ldq`` (a 16-byte multiple) but not their alignment, so
    the kernel's loads and stores take different paths (vec_in != vec_out)."""
    case = br.CASE[name]
    bp, G, yp = _pack(case)
    m, nv, nr = case.nv + case.nr, case.nv, case.nr
    B = br.rows_per_iter(m) + 1
    ld = ((m + 3) & ~3) + 4
    q0, gy = _inputs(case, B, dtype, "edges")
    qbuf = torch.full((B * ld + 4,), float("nan"), dtype=dtype, device=DEV)
    gbuf = torch.full((B * ld + 4,), -123.0, dtype=dtype, device=DEV)
    q = qbuf[off_q:off_q + B * ld].view(B, ld)
    gq = gbuf[off_g:off_g + B * ld].view(B, ld)
    q[:, :m] = q0
    assert (q.data_ptr() % 16 == 0) == (off_q == 0) and (gq.data_ptr() % 16 == 0) == (off_g == 0)
    _, lse = ops.bar_forward_raw(q, bp)
    fn = getattr(_lib.load(), "rayen_bar_backward_f32" if dtype == torch.float32 else "rayen_bar_backward_f64")
    with torch.cuda.device(0):
        _lib.check(fn(bp.handle, q.data_ptr(), ld, lse.data_ptr(), gy.data_ptr(), B, gq.data_ptr(), ops._stream(0)), "bar_backward")
        torch.cuda.synchronize()
    tol = br.tolerance_factor(case) * br.U[dtype]
    q64, gy64 = q[:, :m].double(), gy.double()
    eb = br.scaled_err(gq[:, :m], br.backward64(G, nv, nr, q64, gy64), br.backward_scale(G, nv, nr, q64, gy64)).max().item()
    print(f"{name} {str(dtype)[6:]} q+{off_q} grad_q+{off_g}: backward {eb / tol:.3f} of C u")
    assert eb <= tol
    assert torch.all(gq[:, m:] == -123.0) and torch.all(gbuf[:off_g] == -123.0) and torch.all(gbuf[off_g + B * ld:] == -123.0)


# ------------------------------------------------------------------------------------------------------------------
# large logits: the bar is torch's own working-precision evaluation of the formula
# ------------------------------------------------------------------------------------------------------------------

LARGE = ["L16_k4_wide", "L16_k8_thousand_generators", "L16_k16_sixteen_pieces", "L16_k32_one_ray", "L16_k64_simplex_like"]


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("amplitude", [1e2, 1e3, 1e4])
@pytest.mark.parametrize("name", LARGE)
def test_large_logits_forward_and_backward(name, amplitude, dtype):
    """Logits uniform in +-amplitude, B = 4 096.  The kernel must be within 4 x the scaled error of the same formula
    in plain torch ops of the working precision (softmax, abs, matmul, autograd), with a floor of 16 u.

    Measured on an MI355X, fp32 backward, kernel error / torch error: see DESIGN.md section 9."""
    case = br.CASE[name]
    bp, G, yp = _pack(case)
    k, nv, nr = case.k, case.nv, case.nr
    B, u = 4096, br.U[dtype]
    q, gy = _inputs(case, B, dtype, "plain", amplitude)
    y, lse = ops.bar_forward_raw(q, bp)
    gq = ops.bar_backward_raw(q, lse, gy, bp)
    leaf = q.clone().requires_grad_(True)
    w = torch.cat([torch.softmax(leaf[:, :nv], dim=1), torch.abs(leaf[:, nv:])], dim=1)
    yt = w @ G.to(dtype).t() + yp.to(dtype)
    yt.backward(gy)
    q64, gy64 = q.double(), gy.double()
    yref, S = br.forward64(G, yp, nv, nr, q64), br.forward_scale(G, yp, nv, nr, q64)
    gref, T = br.backward64(G, nv, nr, q64, gy64), br.backward_scale(G, nv, nr, q64, gy64)
    res = {}
    for direction, got, torch_got, ref, scale in (("forward", y, yt.detach(), yref, S), ("backward", gq, leaf.grad, gref, T)):
        ek = br.scaled_err(got, ref, scale).max().item()
        et = br.scaled_err(torch_got, ref, scale).max().item()
        res[direction] = (ek, et)
        print(f"{name} {str(dtype)[6:]} K={br.pad_k(k)} +-{amplitude:g} {direction}: kernel {ek:.3e} torch {et:.3e} "
              f"ratio {ek / et if et else float('inf'):.2f} (in u: {ek / u:.1f} / {et / u:.1f})")
    for direction, (ek, et) in res.items():
        assert ek <= max(4 * et, 16 * u), (name, amplitude, direction, ek, et)
    assert torch.isfinite(y).all() and torch.isfinite(gq).all()


# ------------------------------------------------------------------------------------------------------------------
# capacity: the 160 KiB of LDS
# ------------------------------------------------------------------------------------------------------------------

def _largest_m(K, elem):
    m = (br.LDS_BUDGET // (K * elem) - 1) & ~3
    assert br.lds_bytes(m, K, elem) <= br.LDS_BUDGET < br.lds_bytes(m + 4, K, elem)
    return m


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("K", [4, 16, 64])
def test_largest_image_is_served_and_the_next_is_refused(K, dtype):
    elem = 4 if dtype == torch.float32 else 8
    m = _largest_m(K, elem)
    case = br.Case(f"capacity_K{K}_m{m}", K, m - 5, 5)
    q, gy = _inputs(case, 1000, dtype)
    _check(case, q, gy, "largest image")
    _pack.cache_clear()

    over = br.Case(f"capacity_K{K}_m{m + 4}", K, m - 1, 5)
    G, yp = br.make_pack(over)
    bp = ops.BarPack(G, yp, over.nv, over.nr, 0)
    B = 8
    q = torch.zeros(B, m + 4, dtype=dtype, device=DEV)
    y = torch.full((B, K), -123.0, dtype=dtype, device=DEV)
    gq = torch.full((B, m + 4), -123.0, dtype=dtype, device=DEV)
    lse = torch.zeros(B, dtype=dtype, device=DEV)
    gy = torch.ones(B, K, dtype=dtype, device=DEV)
    tag = "f32" if dtype == torch.float32 else "f64"
    lib = _lib.load()
    with torch.cuda.device(0):
        rc_f = getattr(lib, "rayen_bar_forward_" + tag)(bp.handle, q.data_ptr(), B, m + 4, y.data_ptr(), K, lse.data_ptr(),
                                                        bp.nan_flag.data_ptr(), ops._stream(0))
        rc_b = getattr(lib, "rayen_bar_backward_" + tag)(bp.handle, q.data_ptr(), m + 4, lse.data_ptr(), gy.data_ptr(), B,
                                                         gq.data_ptr(), ops._stream(0))
        torch.cuda.synchronize()
    assert rc_f == _lib.E_UNSUPPORTED and rc_b == _lib.E_UNSUPPORTED
    assert torch.all(y == -123.0) and torch.all(gq == -123.0)                # nothing was launched
    with pytest.raises(_lib.RayenError) as err:
        ops.bar_forward_raw(q, bp)
    assert err.value.code == _lib.E_UNSUPPORTED
    bp.close()


def _box11():
    raw = workloads._empty(11)
    raw["A1"], raw["b1"] = np.r_[np.eye(11), -np.eye(11)], np.ones((22, 1))
    layer = ConstraintModule(workloads.build_constraints(raw), method="Bar", create_map=False).to(DEV)
    assert layer.num_vertices == 2048 and layer.num_rays == 0 and layer.k == 11
    return layer


def _module_G(layer):
    n = layer.n
    gens = torch.cat([X.double().reshape(n, -1) for X in (layer.V, layer.R) if X.numel()], dim=1)
    return layer.NA_E.double() @ gens, layer.yp.double().reshape(-1)


def _module_err(layer, q, y):
    G, yp = _module_G(layer)
    nv, nr = layer.num_vertices, layer.num_rays
    q64 = q[:, :, 0].double()
    return br.scaled_err(y[:, :, 0], br.forward64(G, yp, nv, nr, q64), br.forward_scale(G, yp, nv, nr, q64)).max().item()


def test_a_pack_that_fits_in_fp32_only_is_refused_in_fp64_under_strict(monkeypatch):
    """The 11-D box: 2 048 vertices at K = 16 are 131 KiB of fp32 and 262 KiB of fp64."""
    layer = _box11()
    monkeypatch.setattr(layer, "_bar_reference", lambda *a, **k: (_ for _ in ()).throw(AssertionError("eager detour")))
    q = torch.empty(300, 2048, 1, device=DEV).uniform_(-5, 5)
    case = br.Case("box11", 11, 2048, 0)
    assert _module_err(layer, q, layer(q)) <= br.tolerance_factor(case) * br.U[torch.float32]
    with pytest.raises(_lib.RayenError) as err:
        layer(q.double())
    assert err.value.code == _lib.E_UNSUPPORTED


@pytest.mark.eager_detour
def test_a_pack_that_fits_in_fp32_only_detours_loudly_in_fp64(monkeypatch):
    monkeypatch.delenv("RAYEN_STRICT_HIP", raising=False)
    layer = _box11()
    q = torch.empty(300, 2048, 1, device=DEV).uniform_(-5, 5)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        y64 = layer(q.double())
        layer(q.double())
    ours = [w for w in seen if "rayen_amd" in str(w.message)]
    assert len(ours) == 1 and issubclass(ours[0].category, RuntimeWarning)
    # the detour IS torch's op sequence: equal to the same ops evaluated here; torch's own fp64 softmax of a 2 048-wide
    # row is good to about 5e-10 on the device (bar_reference.softmax64), hence the second, looser line
    G, yp = _module_G(layer)
    torch_formula = (torch.softmax(q[:, :, 0].double(), dim=1) @ G.t() + yp).unsqueeze(2)
    assert y64.dtype == torch.float64 and _module_err(layer, q.double(), y64) <= 1e-8
    S = br.forward_scale(G, yp, 2048, 0, q[:, :, 0].double())
    assert br.scaled_err(y64[:, :, 0], torch_formula[:, :, 0], S).max().item() <= 1e-12
    calls = []
    real = ops.bar_forward_raw
    monkeypatch.setattr(ops, "bar_forward_raw", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(layer, "_bar_reference", lambda *a, **k: (_ for _ in ()).throw(AssertionError("eager detour")))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y32 = layer(q)
    case = br.Case("box11", 11, 2048, 0)
    assert calls and _module_err(layer, q, y32) <= br.tolerance_factor(case) * br.U[torch.float32]


# ------------------------------------------------------------------------------------------------------------------
# more than one launch: rows that span 4 GiB
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 64])
def test_rows_beyond_4_gib_take_a_second_launch(k):
    """fp32, q a [B, 64] view of a [B, 1 024] buffer just above 4 GiB: the forward splits at row 2^20 (rowstat + r0, y + r0 k);
    the backward gets q at full width, so grad_q is split too (grad_y + r0 k)."""
    free, _ = torch.cuda.mem_get_info()
    if free < 24 << 30:
        pytest.skip(f"needs 24 GiB of free device memory for two 4.3 GiB buffers and their copies, {free >> 30} GiB are free")
    case = br.Case(f"multi_launch_k{k}", k, 40, 24)
    bp, G, yp = _pack(case)
    m, W, B = 64, 1024, (1 << 20) + 4096
    split = (1 << 32) // (W * 4)
    assert B * W * 4 > 1 << 32 and 0 < split < B
    gen = torch.Generator(device=DEV).manual_seed(k)
    buf = torch.full((B, W), float("nan"), device=DEV)
    buf[:, :m] = torch.empty(B, m, device=DEV).uniform_(-5, 5, generator=gen)
    gy = torch.randn(B, k, device=DEV, generator=gen)
    y, lse = ops.bar_forward_raw(buf[:, :m], bp)
    gq = ops.bar_backward_raw(buf, lse, gy, bp)
    rows = torch.cat([torch.arange(0, 64), torch.arange(split - 64, split + 64), torch.arange(B - 64, B),
                      torch.arange(0, B, 4099)]).unique().to(DEV)
    q64, gy64 = buf[rows, :m].double(), gy[rows].double()
    tol = br.tolerance_factor(case) * br.U[torch.float32]
    ef = br.scaled_err(y[rows], br.forward64(G, yp, 40, 24, q64), br.forward_scale(G, yp, 40, 24, q64)).max().item()
    eb = br.scaled_err(gq[rows, :m], br.backward64(G, 40, 24, q64, gy64), br.backward_scale(G, 40, 24, q64, gy64)).max().item()
    lse_ok = torch.all(torch.abs(lse[rows].double() - br.lse64(40, q64)) <= 4 * br.U[torch.float32] * (1 + br.lse64(40, q64).abs()))
    tail_zero = bool(torch.all(gq[rows, m:] == 0))
    del buf, gq, y, lse, gy
    _pack.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()
    print(f"k={k}: {rows.numel()} rows around the launch boundary {split}: forward {ef / tol:.3f} backward {eb / tol:.3f} of C u")
    assert ef <= tol and eb <= tol and lse_ok and tail_zero


# ------------------------------------------------------------------------------------------------------------------
# wrapper and module
# ------------------------------------------------------------------------------------------------------------------

def _module(method):
    if method == "Bar":
        cs = workloads.build_constraints(load_golden("example_08")[0])
    else:
        cs = workloads.build_constraints(workloads.make_raw("c2", seed=3))
    return ConstraintModule(cs, method=method, create_map=False).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind", ["expanded_row", "one_row_with_a_short_stride"])
@pytest.mark.parametrize("method", ["Bar", "RAYEN"])
def test_broadcast_rows_are_served_like_their_dense_copy(method, kind, dtype):
    layer = _module(method)
    m = layer.getDimAfterMap()
    gen = torch.Generator().manual_seed(11)
    base = torch.empty(4 * m + 8, dtype=dtype).uniform_(-1.5, 1.5, generator=gen).to(DEV)
    if kind == "expanded_row":
        x = base[:m].view(1, m, 1).expand(37, m, 1)
        assert x.stride() == (0, 1, 1)
    else:
        x = torch.as_strided(base, (1, m, 1), (1, 1, 1), 3)
        assert x.stride(0) < m or m == 1
    B = x.shape[0]
    gy = torch.randn(B, layer.k, 1, generator=gen, dtype=dtype).to(DEV)
    dense = x.detach().clone(memory_format=torch.contiguous_format)
    assert dense.stride() == (m, 1, 1)
    with torch.no_grad():
        assert torch.equal(layer(x), layer(dense))
    a = x.detach().requires_grad_(True)                        # (detach keeps the strides)
    assert a.stride() == x.stride()
    d = dense.requires_grad_(True)
    ya, yd = layer(a), layer(d)
    assert torch.equal(ya, yd)
    ya.backward(gy)
    yd.backward(gy)
    assert a.grad is not None and torch.equal(a.grad, d.grad) and torch.isfinite(d.grad).all() and d.grad.abs().sum() > 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], **_ids)
def test_half_precision_activations_forward_and_backward(dtype):
    """16-bit activations are computed in fp32 and rounded once: value and gradient lie within the 16-bit type's own u
    (plus the fp32 sweep's bar) of the formula on the up-cast input, in the scaled metric."""
    layer = _module("Bar")
    nv, nr, k = layer.num_vertices, layer.num_rays, layer.k
    m = nv + nr
    G, yp = _module_G(layer)
    gen = torch.Generator().manual_seed(5)
    q = torch.empty(1000, m, 1).uniform_(-5, 5, generator=gen).to(DEV).to(dtype).requires_grad_(True)
    gy = torch.randn(1000, k, 1, generator=gen).to(DEV).to(dtype)
    y = layer(q)
    assert y.dtype == dtype
    y.backward(gy)
    assert q.grad is not None and q.grad.dtype == dtype
    q64, gy64 = q.detach()[:, :, 0].double(), gy[:, :, 0].double()
    tol = br.U[dtype] + br.tolerance_factor(br.Case("example_08", k, nv, nr)) * br.U[torch.float32]
    ef = br.scaled_err(y.detach()[:, :, 0], br.forward64(G, yp, nv, nr, q64), br.forward_scale(G, yp, nv, nr, q64)).max().item()
    eb = br.scaled_err(q.grad[:, :, 0], br.backward64(G, nv, nr, q64, gy64), br.backward_scale(G, nv, nr, q64, gy64)).max().item()
    print(f"{dtype}: forward {ef / br.U[dtype]:.3f} u backward {eb / br.U[dtype]:.3f} u")
    assert ef <= tol and eb <= tol
