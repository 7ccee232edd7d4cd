"""method='Bar' on the MI355X: rayen_bar.hip forward / backward against the fp64 torch formula, NaN handling, graph
capture and routing (the suite's conftest runs every test here under RAYEN_STRICT_HIP=1)."""
import numpy as np
import pytest
import torch

from helpers import load_golden
from rayen_amd import ops, workloads
from rayen_amd.constraint_module import ConstraintModule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _raw_lin(A, b, k):
    raw = workloads._empty(k)
    raw["A1"], raw["b1"] = A, b
    return raw


def _layer(name):
    if name.startswith("example_"):
        raw = load_golden(name)[0]
    elif name == "box10":
        raw = _raw_lin(np.r_[np.eye(10), -np.eye(10)], np.ones((20, 1)), 10)
    elif name == "simplex64":
        raw = _raw_lin(np.r_[-np.eye(64), np.ones((1, 64))], np.r_[np.zeros(64), [1.0]][:, None], 64)
        raw["y0"] = np.full((64, 1), 1.0 / 128)
    else:  # random 5-D polytope with a few hundred vertices
        rng = np.random.default_rng(5)
        D = rng.normal(size=(60, 5))
        raw = _raw_lin(D / np.linalg.norm(D, axis=1, keepdims=True), np.ones((60, 1)), 5)
    return ConstraintModule(workloads.build_constraints(raw), method="Bar", create_map=False)


SETS = ["example_00", "example_04", "example_06", "example_07", "example_08", "box10", "simplex64", "poly5"]


def _formula64(layer, q):
    nv, nr = layer.num_vertices, layer.num_rays
    q = q.double()
    z = 0
    if nv:
        z = z + layer.V.double() @ torch.softmax(q[:, :nv, None], dim=1)
    if nr:
        z = z + layer.R.double() @ torch.abs(q[:, nv:nv + nr, None])
    return (layer.NA_E.double() @ z + layer.yp.double())[:, :, 0]


def _row_err(y, ref):
    return (torch.max(torch.abs(y.double() - ref), dim=1).values / torch.clamp(torch.max(torch.abs(ref), dim=1).values,
                                                                                 min=1e-30))


@pytest.mark.parametrize("name", SETS)
def test_forward_matches_the_fp64_formula(name):
    layer = _layer(name)
    if name == "poly5":
        assert layer.num_vertices >= 200
    m = layer.getDimAfterMap()
    gen = torch.Generator().manual_seed(7)
    worst = 0.0
    for B in (0, 1, 500, 4097, 262144):
        q = torch.empty(B, m).uniform_(-5.0, 5.0, generator=gen)
        layer64 = _layer(name).double().to(DEV)
        ref = _formula64(layer64, q.double().to(DEV))
        y64 = layer64(q.double().to(DEV).unsqueeze(2))[:, :, 0]
        layer32 = layer.to(DEV)
        y32 = layer32(q.to(DEV).unsqueeze(2))[:, :, 0]
        assert y32.shape == (B, layer.k) and y32.dtype == torch.float32
        if B:
            e64 = _row_err(y64, ref).max().item()
            e32 = _row_err(y32, _formula64(layer32, q.to(DEV))).max().item()
            assert e64 <= 1e-12, (B, e64)
            assert e32 <= 1e-5, (B, e32)
            worst = max(worst, e32)
    print(f"{name}: nv={layer.num_vertices} nr={layer.num_rays} k={layer.k} worst fp32 row error {worst:.3e}")


def test_wide_and_strided_inputs_and_half_precision():
    layer = _layer("example_08").to(DEV)
    m = layer.getDimAfterMap()
    q = torch.randn(1000, m + 5, device=DEV)
    ref = _formula64(layer, q[:, :m])
    assert _row_err(layer(q.unsqueeze(2))[:, :, 0], ref).max().item() <= 1e-5
    qs = torch.randn(m, 777, device=DEV).t()                   # non-contiguous rows
    assert _row_err(layer(qs.unsqueeze(2))[:, :, 0], _formula64(layer, qs)).max().item() <= 1e-5
    yh = layer(q[:, :m].half().unsqueeze(2))
    assert yh.dtype == torch.float16
    assert _row_err(yh[:, :, 0].float(), _formula64(layer, q[:, :m].half().float())).max().item() <= 2e-3


def test_huge_logits_give_no_nan_and_a_nan_input_asserts():
    layer = _layer("example_08").to(DEV)
    m = layer.getDimAfterMap()
    q = torch.empty(4096, m, device=DEV).uniform_(-1e4, 1e4)
    y = layer(q.unsqueeze(2))[:, :, 0]
    assert torch.isfinite(y).all()
    assert _row_err(y, _formula64(layer, q)).max().item() <= 1e-5
    # -inf logits weigh 0 (torch's softmax), also where they fill a lane's first pieces (box10: 16 lanes per row)
    box = _layer("box10").to(DEV)
    qb = torch.randn(2048, box.getDimAfterMap(), device=DEV)
    qb[:, :8] = float("-inf")
    qb[::2, 64:130] = float("-inf")
    yb = box(qb.unsqueeze(2))[:, :, 0]
    assert torch.isfinite(yb).all()
    assert _row_err(yb, _formula64(box, qb)).max().item() <= 1e-5
    q[17, 0] = float("nan")
    with pytest.raises(AssertionError):
        layer(q.unsqueeze(2))
    layer(torch.zeros(8, m, 1, device=DEV))                     # the flag was cleared


@pytest.mark.parametrize("name", ["example_08", "poly5"])
def test_gradcheck_fp64_and_fp32_gradients(name):
    layer = _layer(name).double().to(DEV)
    m = layer.getDimAfterMap()
    _, pack_id = layer.bar_pack(torch.device(DEV))
    q = torch.randn(6, m, dtype=torch.float64, device=DEV, requires_grad=True)
    q.data[q.data.abs() < 1e-3] += 0.01                        # (away from the kink of |.|)
    assert torch.autograd.gradcheck(lambda t: torch.ops.rayen_amd.bar_project(t, pack_id)[0], (q,))

    layer32 = _layer(name).to(DEV)
    x = torch.randn(3000, m + 2, device=DEV)
    gy = torch.randn(3000, layer.k, device=DEV)
    q32 = x.clone().requires_grad_(True)
    layer32(q32.unsqueeze(2))[:, :, 0].backward(gy)
    q64 = x.double().clone().requires_grad_(True)
    _formula64(layer32, q64[:, :m]).backward(gy.double())
    err = (torch.max(torch.abs(q32.grad.double() - q64.grad), dim=1).values
           / torch.clamp(torch.max(torch.abs(q64.grad), dim=1).values, min=1e-30))
    assert err.max().item() <= 1e-5, err.max().item()
    assert torch.all(q32.grad[:, m:] == 0)


def test_gradients_flow_through_a_mapper():
    cs = workloads.build_constraints(load_golden("example_04")[0])
    layer = ConstraintModule(cs, input_dim=6, method="Bar", create_map=True).to(DEV)
    x = torch.randn(256, 6, 1, device=DEV)
    layer(x).square().sum().backward()
    assert layer.mapper.weight.grad is not None and torch.isfinite(layer.mapper.weight.grad).all()
    assert not any(b.requires_grad for b in (layer.V, layer.R))


def test_graph_capture_replays_forward_and_backward():
    layer = _layer("box10").to(DEV)
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
    new_q = torch.randn(4097, m, device=DEV)
    with torch.no_grad():
        static_q.copy_(new_q)
    graph.replay()
    torch.cuda.synchronize()
    eager_q = new_q.clone().requires_grad_(True)
    y = layer(eager_q.unsqueeze(2))[:, :, 0]
    y.backward(static_g)
    assert torch.equal(static_y, y)
    assert torch.equal(static_q.grad, eager_q.grad)


def test_the_module_reaches_the_kernel(monkeypatch):
    layer = _layer("example_00").to(DEV)
    calls = []
    real = ops.bar_forward_raw
    monkeypatch.setattr(ops, "bar_forward_raw", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(layer, "_bar_reference", lambda *a, **k: (_ for _ in ()).throw(AssertionError("eager detour")))
    layer(torch.randn(500, 3, 1, device=DEV))
    q = torch.randn(500, 3, 1, device=DEV, requires_grad=True)
    layer(q).sum().backward()
    assert calls and q.grad is not None and not layer._hip_unsupported
