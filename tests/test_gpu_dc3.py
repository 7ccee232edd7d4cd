"""method='DC3' on the MI355X: rayen_dc3.hip forward / backward against the reference's own outputs (fixtures under
tests/golden/dc3, from the real reference), the batch-global stop, graph capture, NaN handling and routing (the suite's
conftest runs every test here under RAYEN_STRICT_HIP=1).

Bars: the error of ``y`` and of ``grad_q`` against the reference's fp64 values, per row and relative to the row's largest
magnitude, is at most 4 x the reference-fp32-versus-reference-fp64 error of the same case (read from the fixture), with the
golden floors 1e-5 (fp32) and 1e-11 (fp64).  The factor 4 is the allowance tests/test_gpu_bar_sweep.py gives for a different
summation order; here it also covers that difference compounding over the steps."""
import warnings

import numpy as np
import pytest
import torch

import dc3_cases
from rayen_amd import _lib, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = {torch.float32: 1e-5, torch.float64: 1e-11}


def _bar(z, key, mode, dtype):
    ref_gap = dc3_cases.row_err(z[f"{key}32_{mode}"], z[f"{key}64_{mode}"]).max() if dtype == torch.float32 else 0.0
    return max(4.0 * ref_gap, FLOOR[dtype])


@pytest.mark.parametrize("mode", dc3_cases.MODES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", dc3_cases.NAMES)
def test_fixture_case(name, dtype, mode):
    layer, z = dc3_cases.layer_for(name, dtype)
    layer = layer.to(DEV)
    layer.train(mode == "train")
    tag = "32" if dtype == torch.float32 else "64"
    q = torch.tensor(z["q"]).to(dtype).to(DEV).requires_grad_(True)
    y = layer(q)
    steps = int(layer.dc3_steps.item())
    (torch.tensor(z["w"]).to(dtype).to(DEV).unsqueeze(2) * y).sum().backward()
    with torch.no_grad():
        y_inf = layer(q.detach())                 # the plain-inference route (straight to the C ABI)
    ey = dc3_cases.row_err(y.detach().cpu()[:, :, 0], z[f"y64_{mode}"]).max()
    eg = dc3_cases.row_err(q.grad.cpu()[:, :, 0], z[f"gq64_{mode}"]).max()
    by, bg = _bar(z, "y", mode, dtype), _bar(z, "gq", mode, dtype)
    print(f"{name} {tag} {mode}: steps {steps} (fixture {int(z[f'steps{tag}_{mode}'])})  y err {ey:.3e} bar {by:.3e} "
          f"ratio {ey / by:.3f}  grad err {eg:.3e} bar {bg:.3e} ratio {eg / bg:.3f}")
    assert y.shape == (q.shape[0], layer.k, 1) and y.dtype == dtype
    assert steps == int(z[f"steps{tag}_{mode}"])
    assert torch.equal(y_inf, y.detach())
    assert ey <= by
    assert eg <= bg
    assert not layer._hip_unsupported


def _cube_layer(dtype=torch.float64, **over):
    args = dict(lr=1e-2, momentum=0.5, eps_converge=1e-3, max_steps_training=10, max_steps_testing=400)
    args.update(over)
    previous = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        layer = ConstraintModule(workloads.build_constraints(workloads.cube()), method="DC3", create_map=False, args_DC3=args)
    finally:
        torch.set_default_dtype(previous)
    return layer.to(DEV).eval()


def _reference(layer, q):
    from rayen_amd import dc3
    y, steps = dc3.reference_forward(layer, q, return_steps=True)
    return y, steps


@pytest.mark.parametrize("B", [0, 1, 255, 257, 65537])
def test_batch_sizes_and_wide_rows(B):
    layer = _cube_layer(eps_converge=0.05, max_steps_testing=70)
    gen = torch.Generator().manual_seed(B)
    q = torch.empty(B, 3 + 5, dtype=torch.float64).uniform_(-1.0, 2.0, generator=gen).to(DEV)     # ldq wider than n
    y = layer(q.unsqueeze(2))
    assert y.shape == (B, 3, 1)
    if B == 0:
        return
    ref, steps = _reference(layer, q[:, :3].unsqueeze(2))
    assert int(layer.dc3_steps.item()) == steps
    assert dc3_cases.row_err(y.cpu()[:, :, 0], ref.cpu()[:, :, 0]).max() <= 1e-11
    qg = q.clone().requires_grad_(True)
    layer(qg.unsqueeze(2)).square().sum().backward()
    qr = q[:, :3].clone().requires_grad_(True)
    _reference(layer, qr.unsqueeze(2))[0].square().sum().backward()
    assert dc3_cases.row_err(qg.grad.cpu()[:, :3], qr.grad.cpu()).max() <= 1e-11
    assert torch.all(qg.grad[:, 3:] == 0)
    qs = q[:, :3].t().contiguous().t()                        # non-contiguous rows
    assert torch.equal(layer(qs.unsqueeze(2)), y)


def test_one_outlier_row_delays_the_stop_for_every_row():
    layer = _cube_layer(max_steps_testing=2000)
    gen = torch.Generator().manual_seed(11)
    q = torch.empty(5000, 3, dtype=torch.float64).uniform_(-0.05, 1.05, generator=gen).to(DEV)
    y_near = layer(q.unsqueeze(2))
    steps_near = int(layer.dc3_steps.item())
    q_out = q.clone()
    q_out[4321] = torch.tensor([9.0, -7.0, 5.0], dtype=torch.float64)
    y_out = layer(q_out.unsqueeze(2))
    steps_out = int(layer.dc3_steps.item())
    ref, steps_ref = _reference(layer, q_out.unsqueeze(2))
    assert steps_out == steps_ref and 1 <= steps_near < steps_out < 2000
    assert dc3_cases.row_err(y_out.cpu()[:, :, 0], ref.cpu()[:, :, 0]).max() <= 1e-11
    # the other rows kept being corrected while the outlier converged: the rule is global, not per row
    others = torch.arange(5000, device=DEV) != 4321
    assert not torch.equal(y_out[others], y_near[others])


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_graph_capture_replays_the_eager_bits(training):
    # Inputs from U(-0.5, 0.5): at the fixture's lr the reference's own iteration overflows on 16 of 4097 rows of U(-1, 1)
    # (checked with the torch formula on the host).  Half the fixture's eps makes eval mode stop at about 60 steps: two
    # launches of steps and a replay from the saved state.
    _, fixture_args, _ = dc3_cases.load("dc3_c2")
    layer, z = dc3_cases.layer_for("dc3_c2", args=dict(fixture_args, eps_converge=0.5 * fixture_args["eps_converge"]))
    layer = layer.to(DEV)
    layer.train(training)
    n = layer.n
    gen = torch.Generator().manual_seed(21)
    static_q = (torch.rand(4097, n, generator=gen) - 0.5).to(DEV).requires_grad_(True)
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
    new_q = (torch.rand(4097, n, generator=gen) - 0.5).to(DEV)
    with torch.no_grad():
        static_q.copy_(new_q)
    graph.replay()
    torch.cuda.synchronize()
    eager_q = new_q.clone().requires_grad_(True)
    y = layer(eager_q.unsqueeze(2))[:, :, 0]
    steps = int(layer.dc3_steps.item())
    y.backward(static_g)
    assert steps == 10 if training else 32 < steps <= 64, steps
    assert torch.equal(static_y, y)
    assert torch.equal(static_q.grad, eager_q.grad)


def test_nan_input_raises_the_reference_assertion_and_half_inputs_run_in_fp32():
    layer, z = dc3_cases.layer_for("dc3_cube")
    layer = layer.to(DEV).eval()
    q = torch.tensor(z["q"]).to(DEV)
    yh = layer(q.half())
    assert yh.dtype == torch.float16
    assert dc3_cases.row_err(yh.float().cpu()[:, :, 0], layer(q.half().float()).cpu()[:, :, 0]).max() <= 2e-3
    bad = q.clone()
    bad[7, 1, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"args_DC3\['lr'\]"):
        layer(bad)
    layer(q)                                                   # the flag was cleared


def test_the_module_reaches_the_kernel_and_gradients_flow_through_a_mapper(monkeypatch):
    raw, args, z = dc3_cases.load("dc3_corridor")
    torch.manual_seed(5)                                        # (the mapper's weights)
    layer = ConstraintModule(workloads.build_constraints(raw), input_dim=7, method="DC3", args_DC3=args).to(DEV)
    calls = []
    real = ops.dc3_forward_raw
    monkeypatch.setattr(ops, "dc3_forward_raw", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(layer, "_dc3_reference", lambda *a, **k: (_ for _ in ()).throw(AssertionError("eager detour")))
    # (small inputs: at the fixture's lr the reference's own iteration overflows on some rows of U(-1, 1))
    x = (0.25 * torch.randn(300, 7, 1, generator=torch.Generator().manual_seed(31))).to(DEV)
    layer(x).square().sum().backward()
    assert calls and layer.mapper.weight.grad is not None and torch.isfinite(layer.mapper.weight.grad).all()
    assert not layer._hip_unsupported


def test_backward_workspace_limit_is_a_clear_error(monkeypatch):
    layer = _cube_layer()
    monkeypatch.setattr(ops, "DC3_MAX_WORKSPACE_BYTES", 1 << 20)
    q = torch.rand(4096, 3, dtype=torch.float64, device=DEV, requires_grad=True)
    y = layer(q.unsqueeze(2))
    with pytest.raises(RuntimeError, match="DC3_MAX_WORKSPACE_BYTES"):
        y.sum().backward()


@pytest.mark.eager_detour
def test_a_set_too_large_for_lds_takes_the_announced_detour(monkeypatch):
    raw = workloads.random_lin_quad_soc(k=64, m=700, n_quad=0, n_soc=0, seed=4)      # 700 x 64 fp32 = 175 KiB
    args = dict(lr=1e-4, momentum=0.5, eps_converge=1e-3, max_steps_training=5, max_steps_testing=5)
    layer = ConstraintModule(workloads.build_constraints(raw), method="DC3", create_map=False, args_DC3=args).to(DEV)
    q = torch.rand(64, 64, 1, device=DEV) - 0.5
    monkeypatch.setenv("RAYEN_STRICT_HIP", "1")
    with pytest.raises(_lib.RayenError):
        layer(q)
    monkeypatch.delenv("RAYEN_STRICT_HIP")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        y = layer(q)
        layer(q)
    said = [w for w in seen if issubclass(w.category, RuntimeWarning) and "no HIP kernel serves this DC3" in str(w.message)]
    assert len(said) == 1 and layer._hip_unsupported
    assert torch.equal(y, layer._dc3_reference(q))
