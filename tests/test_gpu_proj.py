"""The Euclidean-projection kernels (rayen_amd/csrc/rayen_proj.hip) through the ops and through ``ProjectionModule`` on
the device, against the fp64 reference of tests/proj_reference.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import proj_reference as pr                                  # noqa: E402
from rayen_amd import _lib, ops, projection                  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in pr.CASES]
DTYPES = ["float32", "float64"]


def _pack(name):
    return ops.ProjPack(pr.module_for(name).program.arrays(), torch.cuda.current_device())


def _inputs(name, dtype_name, B):
    cs = pr.make_cs(name)
    q, gy = pr.make_inputs(name)
    dtype = getattr(torch, dtype_name)
    return (torch.from_numpy(q[:B]).to(dtype).cuda(), torch.from_numpy((gy @ cs.NA_E)[:B]).to(dtype).cuda())


# every case at every precision the kernel stages it at (n64_c3_shape: fp32 only, its fp64 image is over the LDS limit)
SERVED = [(name, dtype_name) for name in NAMES for dtype_name in DTYPES if pr.case_served(name, dtype_name)]


@pytest.mark.parametrize("B", pr.BATCHES)
@pytest.mark.parametrize("name,dtype_name", SERVED)
def test_ops_against_the_reference(name, dtype_name, B):
    pack = _pack(name)
    q, g = _inputs(name, dtype_name, B)
    eps = pr.EPS[dtype_name]
    z, iters, vstar = ops.proj_forward_raw(q, pack, pr.MAX_ITERS, eps)
    grad = ops.proj_backward_raw(g, vstar, iters, pack, pr.MAX_ITERS, eps)
    run = pr.mirror_run(name, dtype_name)
    print(f"{name} {dtype_name} B={B}: fwd gap {pr.row_gap(z.cpu().numpy(), pr.reference(name).z[:B]).max():.3e} "
          f"bwd gap {pr.row_gap(grad.cpu().numpy(), pr.reference(name).grad_q[:B])[~pr.reference(name).kink[:B]].max():.3e} "
          f"iters max {int(iters.max())} mean {float(iters.float().mean()):.1f} (mirror max {int(run.iters[:B].max())}) "
          f"bars {pr.bars(name, dtype_name)}")
    assert pr.compare(name, dtype_name, z.cpu().numpy(), grad.cpu().numpy(), iters.cpu().numpy(), rows=B) == []
    # device and host mirror: the same iteration, so the same answer to the sum of both bars and nearly the same counts
    fwd_bar, bwd_bar, _ = pr.bars(name, dtype_name)
    assert np.all(pr.row_gap(z.cpu().numpy(), run.z[:B]) <= 2 * fwd_bar)
    assert int(iters.max()) < pr.MAX_ITERS


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_module_on_device_trains(dtype_name):
    name = "k8_n5_ragged_equalities"
    cs, ref = pr.make_cs(name), pr.reference(name)
    dtype = getattr(torch, dtype_name)
    layer = projection.ProjectionModule(cs, create_map=False, max_iters=pr.MAX_ITERS, eps=pr.EPS[dtype_name]).to(dtype).cuda()
    q = torch.from_numpy(ref.q.copy()).to(dtype).cuda().requires_grad_(True)
    z, iters = layer.project(q)
    (z * torch.from_numpy(ref.gy @ cs.NA_E).to(dtype).cuda()).sum().backward()
    assert pr.compare(name, dtype_name, z.detach().cpu().numpy(), q.grad.cpu().numpy(), iters.cpu().numpy()) == []
    y = layer(q.detach())
    assert y.shape == (pr.BATCH, cs.k, 1)
    assert torch.allclose(y[:, :, 0], z.detach() @ layer.NA_E.T + layer.yp.T, rtol=0, atol=1e-5)
    torch.manual_seed(0)
    net = projection.ProjectionModule(cs, input_dim=6, mode='PP').cuda()
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    x, target = torch.randn(64, 6, device="cuda"), torch.from_numpy(ref.z[:64] @ cs.NA_E.T + cs.yp.T).float().cuda()
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = ((net(x)[:, :, 0] - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0] and np.isfinite(losses).all()
    assert float(np.max(cs.getViolationRows(net(x)[:, :, 0].detach().double().cpu().numpy()))) <= 1e-3
    yb, dist = cs.projectBatch(torch.from_numpy(ref.q[:9] @ cs.NA_E.T + cs.yp.T).to(dtype).cuda())
    assert np.max(np.abs(yb.cpu().numpy() - (ref.z[:9] @ cs.NA_E.T + cs.yp.T))) <= 1e-3 and dist.shape == (9,)


@pytest.mark.parametrize("max_iters", [5, pr.CHUNK, pr.CHUNK + 1, 3 * pr.CHUNK])
def test_iteration_cap_and_chunk_boundaries(max_iters):
    """Rows that need more than ``max_iters`` end AT the cap and say so; the others are untouched by it.  32 ends exactly
    at a launch boundary, 33 and 96 span several launches."""
    name, dtype_name = "n16_four_quadratics", "float32"
    pack = _pack(name)
    q, _ = _inputs(name, dtype_name, 65)
    full = pr.mirror_run(name, dtype_name).iters[:65]
    z, iters, _ = ops.proj_forward_raw(q, pack, max_iters, pr.EPS[dtype_name])
    iters = iters.cpu().numpy()
    assert iters.max() == max_iters and np.any(full > max_iters)
    late = full > max_iters + 2
    assert np.all(iters[late] == max_iters)
    early = full < max_iters - 2
    assert np.all(np.abs(iters[early] - full[early]) <= 2)
    c = pr.module_for(name).constants(torch.float32, torch.device("cpu"))
    zm, im, _ = projection.mirror_forward(c, q.cpu(), max_iters, pr.EPS[dtype_name])
    assert torch.all(torch.isfinite(z))
    assert np.all(pr.row_gap(z.cpu().numpy(), zm.numpy()) <= 1e-4)


def test_strided_input_and_graph_capture():
    name, dtype_name = "k8_n5_ragged_equalities", "float32"
    pack = _pack(name)
    q, _ = _inputs(name, dtype_name, 65)
    wide = torch.full((65, q.shape[1] + 3), 7.0, device="cuda")
    wide[:, :q.shape[1]] = q
    z0, it0, _ = ops.proj_forward_raw(q, pack, 100, 1e-6)
    z1, it1, _ = ops.proj_forward_raw(wide, pack, 100, 1e-6)                 # ldq > n
    assert torch.equal(z0, z1) and torch.equal(it0, it1)
    static_q = q.clone()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.proj_forward_raw(static_q, pack, 100, 1e-6)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            zg, itg, _ = ops.proj_forward_raw(static_q, pack, 100, 1e-6)
    static_q.copy_(q.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(zg, z0.flip(0)) and torch.equal(itg, it0.flip(0))


def test_image_at_the_lds_limit_and_just_over():
    at = pr.module_for(pr.LDS_AT_LIMIT.name)
    cs = pr.make_cs(pr.LDS_AT_LIMIT.name)
    q = torch.from_numpy(pr.make_inputs(pr.LDS_AT_LIMIT.name)[0][:65]).float().cuda()
    pack = ops.ProjPack(at.program.arrays(), torch.cuda.current_device())
    z, iters, _ = ops.proj_forward_raw(q, pack, pr.MAX_ITERS, 1e-6)
    zm, _ = at.project(q.cpu(), max_iters=pr.MAX_ITERS, eps=1e-6)
    assert np.all(pr.row_gap(z.cpu().numpy(), zm.numpy()) <= 1e-4) and int(iters.max()) < pr.MAX_ITERS
    assert float(np.max(cs.getViolationRows(z.double().cpu().numpy()))) <= 1e-3
    over = ops.ProjPack(pr.module_for(pr.LDS_JUST_OVER.name).program.arrays(), torch.cuda.current_device())
    with pytest.raises(_lib.RayenError) as err:
        ops.proj_forward_raw(q, over, 10, 1e-6)
    assert err.value.code == _lib.E_UNSUPPORTED
    layer = projection.ProjectionModule(pr.make_cs(pr.LDS_JUST_OVER.name), create_map=False).cuda()
    with pytest.raises(_lib.RayenError):                     # gpu tests run strict: no detour
        layer.project(q)
