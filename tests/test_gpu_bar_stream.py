"""The streamed Bar kernels (rayen_amd/csrc/rayen_bar_stream.hip: forward / backward x fp32 / fp64 x K in
{4, 8, 16, 32, 64}, the image of G brought through LDS in windows).

Where the resident kernels (rayen_bar.hip) serve a pack the streamed ones must give the SAME BITS: every lane does the
same operations on the same operands in the same order, whatever the window size.  That equality is the oracle of the first
half.  Beyond the resident envelope the oracle is the fp64 reference of tests/bar_reference.py under the existing sweep's
derived bar ``C u``, ``C = 4 ceil(pieces / L) + K + 48``: it bounds a lane's chain length, which the streamed walk does not
change.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

import bar_reference as br
import bar_stream_cases as S
from rayen_amd import _lib, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
_ids = {"ids": lambda v: v.name if isinstance(v, br.Case) else str(v).replace("torch.", "")}


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


@functools.lru_cache(maxsize=None)
def _pack(case):
    G, yp = br.make_pack(case)
    return ops.BarPack(G, yp, case.nv, case.nr, 0), _dev(G), _dev(yp)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _inputs(case, B, dtype, variant="plain"):
    q, gy = br.make_inputs(case, B, variant)
    return _dev(q, dtype), _dev(gy, dtype)


def _both(q, gy, bp, kernel, window=0):
    y, lse = ops.bar_forward_raw(q, bp, kernel=kernel, window_bytes=window)
    return y, lse, ops.bar_backward_raw(q, lse, gy, bp, kernel=kernel, window_bytes=window)


def _assert_same_bits(case, q, gy, bp, window, what, resident=None):
    """Streamed at ``window`` against the default route on the same input: y, rowstat and grad_q bit for bit (grad_q on
    [:, :m], where the inputs are NaN-free; exactly 0 beyond)."""
    m = case.nv + case.nr
    y0, lse0, gq0 = resident if resident is not None else _both(q, gy, bp, "resident")
    y1, lse1, gq1 = _both(q, gy, bp, "stream", window)
    assert y1.shape == y0.shape and gq1.shape == q.shape and y1.dtype == q.dtype and gq1.dtype == q.dtype
    assert torch.equal(y1, y0), (case.name, what, "y", (y1 != y0).sum().item())
    assert torch.equal(lse1, lse0), (case.name, what, "rowstat")
    assert not torch.isnan(gq0[:, :m]).any()
    assert torch.equal(gq1[:, :m], gq0[:, :m]), (case.name, what, "grad_q", (gq1[:, :m] != gq0[:, :m]).sum().item())
    if q.shape[1] > m:
        assert torch.all(gq1[:, m:] == 0)


# ------------------------------------------------------------------------------------------------------------------
# 1. bit equality where both routes serve
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("case", br.CASES, **_ids)
def test_streamed_equals_resident_bit_for_bit(case, dtype):
    """Windows of one group, of three groups, of the whole image (where a legal window holds it, else the largest legal
    one) and the default x B in {1, rows_per_iter - 1, rows_per_iter + 1} x plain logits and the -inf / zero variant."""
    bp, _, _ = _pack(case)
    windows = S.forced_windows(case, _name(dtype))
    assert (S.window_count(case, _name(dtype), windows[2]) == 1) == S.whole_image_fits(case, _name(dtype))
    assert bp.resident_served(dtype)
    for B in br.sweep_batches(case):
        for variant in ("plain", "edges"):
            q, gy = _inputs(case, B, dtype, variant)
            resident = _both(q, gy, bp, "resident")
            for window in windows:
                _assert_same_bits(case, q, gy, bp, window, f"{variant} B={B} window={window}", resident)


# ------------------------------------------------------------------------------------------------------------------
# 2. several passes per workgroup
# ------------------------------------------------------------------------------------------------------------------

BIG = ["L1_k4_mixed_piece_one_ray", "L2_k5_mixed_piece", "L4_k16_mixed_piece", "L8_k17_six_pieces", "L8_k32_rays_only",
       "L16_k33_ten_pieces", "L16_k64_simplex_like", "L16_k8_thousand_generators"]          # (the existing sweep's)


def _device_inputs(case, B, dtype, seed):
    """Like ``bar_reference.make_inputs(.., 'edges')``, drawn on the device (these batches are large)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    m, nv = case.nv + case.nr, case.nv
    q = torch.empty(B, m, dtype=dtype, device=DEV).uniform_(-5, 5, generator=gen)
    hit = torch.rand(B, m, device=DEV, generator=gen) < 0.25
    if nv > 1:
        hit[torch.arange(B, device=DEV), torch.arange(B, device=DEV) % nv] = False     # one finite vertex logit per row
    else:
        hit[:, :nv] = False
    q[:, :nv][hit[:, :nv]] = float("-inf")
    q[:, nv:][hit[:, nv:]] = 0.0
    return q, torch.randn(B, case.k, dtype=dtype, device=DEV, generator=gen)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("name", BIG)
def test_second_pass_of_a_workgroup(name, dtype):
    """More rows than a full grid takes in one pass, at windows of three groups: every workgroup goes round its window
    sequence again (the last window's step issues the next pass's first copy).  The grid is the launcher's: CUs x the
    workgroups per CU LDS leaves room for (an instance's registers may let fewer be resident at once; the others wait)."""
    case = br.CASE[name]
    m, K, elem = case.nv + case.nr, br.pad_k(case.k), S.ELEM[_name(dtype)]
    window = S.forced_windows(case, _name(dtype))[1]
    rpp = S.rows_per_pass(m, K, dtype == torch.float64)
    wgs = _cus() * S.wg_per_cu(S.lds_bytes(m, S.groups(window, K, elem), K, elem))
    B = wgs * rpp + rpp + 3
    assert B > wgs * rpp
    bp, _, _ = _pack(case)
    q, gy = _device_inputs(case, B, dtype, 7)
    _assert_same_bits(case, q, gy, bp, window, f"second pass B={B}")


# ------------------------------------------------------------------------------------------------------------------
# 3. layouts
# ------------------------------------------------------------------------------------------------------------------

LAYOUT_CASES = ["L2_k5_mixed_piece", "L4_k16_mixed_piece", "L16_k16_sixteen_pieces", "L16_k33_ten_pieces", "L16_k4_wide"]


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("layout", ["stride_m_plus_1", "base_off_by_one_element", "column_stride"])
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_layouts(name, layout, dtype):
    """The existing sweep's three layouts at windows of three groups.  Whatever lies beyond column m is NaN, so a read past
    m poisons y or grad_q."""
    case = br.CASE[name]
    bp, _, _ = _pack(case)
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
    _assert_same_bits(case, q, gy, bp, S.forced_windows(case, _name(dtype))[1], layout)
    y, _, gq = _both(q, gy, bp, "stream", S.forced_windows(case, _name(dtype))[1])
    assert torch.isfinite(y).all() and torch.isfinite(gq[:, :m]).all()


# ------------------------------------------------------------------------------------------------------------------
# 4. beyond the resident envelope, against fp64
# ------------------------------------------------------------------------------------------------------------------

def _check64(case, bp, G, yp, q, gy, what, window=0):
    """The existing sweep's ``_check`` on the streamed route."""
    k, nv, nr = case.k, case.nv, case.nr
    m = nv + nr
    u = br.U[q.dtype]
    tol = br.tolerance_factor(case) * u
    y, lse, gq = _both(q, gy, bp, "stream", window)
    assert y.shape == (q.shape[0], k) and y.dtype == q.dtype and gq.shape == q.shape and gq.dtype == q.dtype
    q64, gy64 = q[:, :m].double(), gy.double()
    ef = br.scaled_err(y, br.forward64(G, yp, nv, nr, q64), br.forward_scale(G, yp, nv, nr, q64)).max().item()
    eb = br.scaled_err(gq[:, :m], br.backward64(G, nv, nr, q64, gy64), br.backward_scale(G, nv, nr, q64, gy64)).max().item()
    print(f"{case.name} {_name(q.dtype)} K={br.pad_k(k)} {what} B={q.shape[0]}: forward {ef / tol:.3f} backward {eb / tol:.3f} "
          f"of C u (C = {tol / u:.0f})")
    assert ef <= tol, (case.name, what, "forward", ef, tol)
    assert eb <= tol, (case.name, what, "backward", eb, tol)
    assert torch.isfinite(y).all() and torch.isfinite(gq[:, :m]).all()
    want = br.lse64(nv, q64)
    assert torch.all(torch.abs(lse.double() - want) <= 4 * u * (1 + want.abs())), (case.name, what, "rowstat")
    dead = torch.isinf(q64) | (q64 == 0)
    assert torch.all(gq[:, :m][dead] == 0)                     # exactly 0 on -inf logits and on zero ray entries


def _largest_m(K, elem):
    m = (br.LDS_BUDGET // (K * elem) - 1) & ~3
    assert br.lds_bytes(m, K, elem) <= br.LDS_BUDGET < br.lds_bytes(m + 4, K, elem)
    return m


def _beyond(case, dtype, min_windows):
    assert S.window_count(case, _name(dtype), 0) >= min_windows
    G, yp = br.make_pack(case)
    bp = ops.BarPack(G, yp, case.nv, case.nr, 0)
    assert not bp.resident_served(dtype)
    with pytest.raises(_lib.RayenError) as err:                # the default route still refuses
        ops.bar_forward_raw(torch.zeros(8, case.nv + case.nr, dtype=dtype, device=DEV), bp)
    assert err.value.code == _lib.E_UNSUPPORTED
    for variant in ("plain", "edges"):
        q, gy = _inputs(case, 1000, dtype, variant)
        _check64(case, bp, _dev(G), _dev(yp), q, gy, variant)
    bp.close()


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("K", [4, 16, 64])
def test_the_first_image_the_resident_kernels_refuse(K, dtype):
    """The ``over`` cases of the existing capacity test: four generators past the largest resident image."""
    m = _largest_m(K, S.ELEM[_name(dtype)])
    _beyond(br.Case(f"capacity_K{K}_m{m + 4}", K, m - 1, 5), dtype, 3)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_three_times_the_resident_envelope(dtype):
    m = 3 * _largest_m(16, S.ELEM[_name(dtype)]) + 7
    _beyond(br.Case(f"beyond_K16_m{m}", 16, m - 5, 5), dtype, 7)


# ------------------------------------------------------------------------------------------------------------------
# 5. modules
# ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _box_cs(d):
    raw = workloads._empty(d)
    raw["A1"], raw["b1"] = np.r_[np.eye(d), -np.eye(d)], np.ones((2 * d, 1))
    return workloads.build_constraints(raw)


def _box(d, **kw):
    layer = ConstraintModule(_box_cs(d), method="Bar", create_map=False, **kw).to(DEV)
    assert layer.num_vertices == 2 ** d and layer.num_rays == 0 and layer.k == d
    return layer


def _no_detour(monkeypatch, layer):
    monkeypatch.setattr(layer, "_bar_reference", lambda *a, **k: (_ for _ in ()).throw(AssertionError("eager detour")))


def _module_G(layer):
    n = layer.n
    gens = torch.cat([X.double().reshape(n, -1) for X in (layer.V, layer.R) if X.numel()], dim=1)
    return layer.NA_E.double() @ gens, layer.yp.double().reshape(-1)


def _module_err(layer, q, y):
    G, yp = _module_G(layer)
    nv, nr = layer.num_vertices, layer.num_rays
    q64 = q[:, :, 0].double()
    return br.scaled_err(y[:, :, 0], br.forward64(G, yp, nv, nr, q64), br.forward_scale(G, yp, nv, nr, q64)).max().item()


def _module_grad_err(layer, q, gy, grad):
    G, _ = _module_G(layer)
    nv, nr = layer.num_vertices, layer.num_rays
    q64, gy64 = q[:, :, 0].double(), gy[:, :, 0].double()
    return br.scaled_err(grad[:, :, 0], br.backward64(G, nv, nr, q64, gy64), br.backward_scale(G, nv, nr, q64, gy64)).max().item()


def _forward_and_backward_within_the_bar(layer, d, dtype, B=300):
    gen = torch.Generator(device=DEV).manual_seed(d)
    q = torch.empty(B, 2 ** d, 1, dtype=dtype, device=DEV).uniform_(-5, 5, generator=gen)
    gy = torch.randn(B, d, 1, dtype=dtype, device=DEV, generator=gen)
    tol = br.tolerance_factor(br.Case(f"box{d}", d, 2 ** d, 0)) * br.U[dtype]
    with torch.no_grad():
        y = layer(q)
    ef = _module_err(layer, q, y)
    leaf = q.clone().requires_grad_(True)
    y2 = layer(leaf)
    assert torch.equal(y2.detach(), y)                         # the registered op runs the code the plain call runs
    y2.backward(gy)
    eb = _module_grad_err(layer, q, gy, leaf.grad)
    print(f"box{d} {_name(dtype)} bar_kernel={layer.bar_kernel}: forward {ef / tol:.3f} backward {eb / tol:.3f} of C u")
    assert ef <= tol and eb <= tol
    return y


@pytest.mark.parametrize("kernel", ["stream", "auto"])
def test_the_12d_box_is_served(kernel, monkeypatch):
    """4 096 vertices at K = 16: 256 KiB of fp32, in neither precision within the resident envelope."""
    layer = _box(12, bar_kernel=kernel)
    _no_detour(monkeypatch, layer)
    _forward_and_backward_within_the_bar(layer, 12, torch.float32)
    bp, _ = layer.bar_pack(torch.device(DEV))
    assert not bp.resident_served(torch.float32) and not bp.resident_served(torch.float64)


def test_the_11d_box_under_auto(monkeypatch):
    """fp32 fits LDS: 'auto' is the resident route, bit for bit the default module.  fp64 does not: streamed."""
    layer, default = _box(11, bar_kernel="auto"), _box(11)
    _no_detour(monkeypatch, layer)
    bp, _ = layer.bar_pack(torch.device(DEV))
    assert layer._bar_kernel_for(bp, torch.float32) == "resident" and layer._bar_kernel_for(bp, torch.float64) == "stream"
    y = _forward_and_backward_within_the_bar(layer, 11, torch.float32)
    gen = torch.Generator(device=DEV).manual_seed(11)
    q = torch.empty(300, 2048, 1, device=DEV).uniform_(-5, 5, generator=gen)
    assert torch.equal(default(q), y)
    _forward_and_backward_within_the_bar(layer, 11, torch.float64)


def test_the_13d_box_takes_an_odd_number_of_windows(monkeypatch):
    """8 192 vertices at K = 16: 512 KiB of fp32.  The default window gives 26 windows; 76 groups a window give 27."""
    layer = _box(13, bar_kernel="stream", bar_window_bytes=76 * 4 * 16 * 4)
    _no_detour(monkeypatch, layer)
    nw = S.window_count(br.Case("box13", 13, 8192, 0), "float32", layer.bar_window_bytes)
    assert nw > 1 and nw % 2 == 1
    _forward_and_backward_within_the_bar(layer, 13, torch.float32)


def test_a_default_12d_module_is_still_refused_under_strict():
    layer = _box(12)
    assert layer.bar_kernel == "resident"
    with pytest.raises(_lib.RayenError) as err:
        layer(torch.zeros(8, 4096, 1, device=DEV))
    assert err.value.code == _lib.E_UNSUPPORTED


@pytest.mark.eager_detour
def test_a_module_switched_to_stream_does_not_inherit_the_resident_refusal(monkeypatch):
    monkeypatch.delenv("RAYEN_STRICT_HIP", raising=False)
    layer = _box(12)
    q = torch.empty(64, 4096, 1, device=DEV).uniform_(-5, 5)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        layer(q)
    assert [w for w in seen if "rayen_amd" in str(w.message)] and layer._refused(q[:, :, 0])
    layer.bar_kernel = "stream"
    assert not layer._refused(q[:, :, 0])
    _no_detour(monkeypatch, layer)
    tol = br.tolerance_factor(br.Case("box12", 12, 4096, 0)) * br.U[torch.float32]
    assert _module_err(layer, q, layer(q)) <= tol


@pytest.mark.parametrize("kernel", ["stream", "auto"])
def test_a_compiled_module_reaches_the_streamed_op(kernel, monkeypatch):
    """torch.compile (backend 'aot_eager': the registered fake implementations and autograd formula, no code generation)
    of the 12-D module: the output and q.grad of the compiled module are the eager module's bits, and the streamed op
    is what ran."""
    import torch._dynamo
    torch._dynamo.reset()
    layer = _box(12, bar_kernel=kernel)
    _no_detour(monkeypatch, layer)
    calls = []
    real = ops.bar_forward_raw
    monkeypatch.setattr(ops, "bar_forward_raw", lambda *a, **k: calls.append(k.get("kernel")) or real(*a, **k))
    gen = torch.Generator(device=DEV).manual_seed(5)
    q = torch.empty(130, 4096, 1, device=DEV).uniform_(-5, 5, generator=gen)
    gy = torch.randn(130, 12, 1, device=DEV, generator=gen)
    eager_q = q.clone().requires_grad_(True)
    y = layer(eager_q)
    y.backward(gy)
    compiled = torch.compile(layer, backend="aot_eager")
    del calls[:]
    for _ in range(2):                                           # (the second call reuses the compiled graph)
        cq = q.clone().requires_grad_(True)
        yc = compiled(cq)
        yc.backward(gy)
        assert torch.equal(yc, y) and torch.equal(cq.grad, eager_q.grad)
    assert calls and set(calls) == {"stream"}
    torch._dynamo.reset()


# ------------------------------------------------------------------------------------------------------------------
# 6. contract
# ------------------------------------------------------------------------------------------------------------------

def test_empty_batch():
    case = br.CASE["L2_k5_mixed_piece"]
    bp, _, _ = _pack(case)
    for dtype in DTYPES:
        q = torch.empty(0, case.nv + case.nr, dtype=dtype, device=DEV)
        y, lse = ops.bar_forward_raw(q, bp, kernel="stream")
        gq = ops.bar_backward_raw(q, lse, torch.empty(0, case.k, dtype=dtype, device=DEV), bp, kernel="stream")
        assert y.shape == (0, case.k) and lse.shape == (0,) and gq.shape == q.shape
    with pytest.raises(ValueError):
        ops.bar_forward_raw(q, bp, kernel="bogus")


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_a_bad_window_is_a_bad_argument_and_launches_nothing(dtype):
    case = br.CASE["L4_k16_mixed_piece"]
    bp, _, _ = _pack(case)
    m, K, B = case.nv + case.nr, 16, 8
    group = 4 * K * S.ELEM[_name(dtype)]
    q = torch.zeros(B, m, dtype=dtype, device=DEV)
    lse = torch.zeros(B, dtype=dtype, device=DEV)
    gy = torch.ones(B, K, dtype=dtype, device=DEV)
    tag = "f32" if dtype == torch.float32 else "f64"
    lib = _lib.load()
    for window in (1000, -16, group - 16, S.DEFAULT_WINDOW + 16):
        y = torch.full((B, K), -123.0, dtype=dtype, device=DEV)
        stat = torch.full((B,), -123.0, dtype=dtype, device=DEV)
        gq = torch.full((B, m), -123.0, dtype=dtype, device=DEV)
        with torch.cuda.device(0):
            rc_f = getattr(lib, "rayen_bar_stream_forward_" + tag)(bp.handle, q.data_ptr(), B, m, y.data_ptr(), K, stat.data_ptr(),
                                                                   bp.nan_flag.data_ptr(), window, ops._stream(0))
            rc_b = getattr(lib, "rayen_bar_stream_backward_" + tag)(bp.handle, q.data_ptr(), m, lse.data_ptr(), gy.data_ptr(), B,
                                                                    gq.data_ptr(), window, ops._stream(0))
            torch.cuda.synchronize()
        assert rc_f == -1 and rc_b == -1, (window, rc_f, rc_b)            # RAYEN_E_BAD_ARG
        assert torch.all(y == -123.0) and torch.all(stat == -123.0) and torch.all(gq == -123.0), window
    with pytest.raises(_lib.RayenError) as err:
        ops.bar_forward_raw(q, bp, kernel="stream", window_bytes=group - 16)
    assert err.value.code == -1
    ops.bar_forward_raw(q, bp, kernel="stream", window_bytes=group)          # one group is the smallest window


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_a_nan_logit_raises_the_flag_as_the_resident_forward_does(dtype):
    case = br.CASE["L16_k33_ten_pieces"]
    bp, _, _ = _pack(case)
    q, _ = _inputs(case, 100, dtype)
    window = S.forced_windows(case, _name(dtype))[1]
    seen = {}
    for poisoned in (False, True):
        if poisoned:
            q[17, 3] = float("nan")
        for kernel in ("resident", "stream"):
            bp.nan_flag.zero_()
            y, _ = ops.bar_forward_raw(q, bp, kernel=kernel, window_bytes=window)
            seen[poisoned, kernel] = (int(bp.nan_flag.item()), torch.isnan(y).any(dim=1))
    bp.nan_flag.zero_()
    assert seen[False, "resident"][0] == seen[False, "stream"][0] == 0
    assert seen[True, "resident"][0] == seen[True, "stream"][0] == 1
    assert torch.equal(seen[True, "resident"][1], seen[True, "stream"][1]) and seen[True, "stream"][1].sum() == 1


def test_graph_capture_replays_forward_and_backward():
    """One forward + backward captured on a single stream and replayed twice equals the eager call (the pack is not
    changed by a call, nothing is allocated by the library)."""
    layer = _box(10, bar_kernel="stream", bar_window_bytes=3 * 4 * 16 * 4)          # three groups a window: 86 windows
    m = layer.getDimAfterMap()
    static_q = torch.randn(4097, m, device=DEV, requires_grad=True)
    static_g = torch.randn(4097, layer.k, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            static_q.grad = None
            layer(static_q.unsqueeze(2))[:, :, 0].backward(static_g)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    static_q.grad = None
    with torch.cuda.graph(graph):
        static_y = layer(static_q.unsqueeze(2))[:, :, 0]
        static_y.backward(static_g)
    for seed in (1, 2):
        new_q = torch.randn(4097, m, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
        with torch.no_grad():
            static_q.copy_(new_q)
        graph.replay()
        torch.cuda.synchronize()
        eager_q = new_q.clone().requires_grad_(True)
        y = layer(eager_q.unsqueeze(2))[:, :, 0]
        y.backward(static_g)
        assert torch.equal(static_y, y)
        assert torch.equal(static_q.grad, eager_q.grad)
    resident = _box(10)
    assert torch.equal(resident(new_q.unsqueeze(2))[:, :, 0], y.detach())       # and the resident route's bits
