"""The PSD block of the Euclidean-projection kernels (rayen_amd/csrc/rayen_proj.hip) through the ops and through
``ProjectionModule(..., lmi=True)`` on the device, against the fp64 reference of tests/proj_lmi_reference.py."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import proj_lmi_reference as L                               # noqa: E402
from rayen_amd import _lib, ops, projection                  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ["float32", "float64"]
# every case at every precision the kernel stages it at (all of them: r32_k4 in fp64 is 143 KiB of LDS)
SERVED = [(c.name, dtype_name) for c in L.CASES for dtype_name in DTYPES if L.case_served(c.name, dtype_name)]


def _pack(name):
    return ops.ProjPack(L.module_for(name).program.arrays(), torch.cuda.current_device())


def _inputs(name, dtype_name, B):
    cs = L.make_cs(name)
    q, gy = L.make_inputs(name)
    dtype = getattr(torch, dtype_name)
    return (torch.from_numpy(q[:B]).to(dtype).cuda(), torch.from_numpy((gy @ cs.NA_E)[:B]).to(dtype).cuda())


def test_every_case_is_served():
    assert len(SERVED) == 2 * len(L.CASES)


@pytest.mark.parametrize("name,dtype_name", SERVED)
def test_ops_against_the_reference(name, dtype_name):
    pack = _pack(name)
    eps = L.EPS[dtype_name]
    run, ref = L.mirror_run(name, dtype_name), L.reference(name)
    for B in L.batches_of(name):
        q, g = _inputs(name, dtype_name, B)
        z, iters, vstar = ops.proj_forward_raw(q, pack, L.MAX_ITERS, eps)
        grad = ops.proj_backward_raw(g, vstar, iters, pack, L.MAX_ITERS, eps)
        zc, gc = z.cpu().numpy(), grad.cpu().numpy()
        print(f"{name} {dtype_name} B={B}: fwd gap {L.row_gap(zc, ref.z[:B]).max():.3e} bwd gap "
              f"{L.row_gap(gc, ref.grad_q[:B])[~ref.kink[:B]].max():.3e} iters max {int(iters.max())} mean "
              f"{float(iters.float().mean()):.1f} (mirror max {int(run.iters[:B].max())}) bars {L.bars(name, dtype_name)}")
        # forward, iters, backward, interior rows unmoved with 0 iterations, violation within its bar
        assert L.compare(name, dtype_name, zc, gc, iters.cpu().numpy(), rows=B) == []
        # device and host mirror: the same iteration, so the same answer to the sum of both bars
        assert np.all(L.row_gap(zc, run.z[:B]) <= 2 * L.bars(name, dtype_name)[0])
        assert int(iters.max()) < L.MAX_ITERS


@pytest.mark.parametrize("name,dtype_name", SERVED)
def test_module_against_the_reference(name, dtype_name):
    cs, ref = L.make_cs(name), L.reference(name)
    dtype = getattr(torch, dtype_name)
    layer = projection.ProjectionModule(cs, create_map=False, max_iters=L.MAX_ITERS, eps=L.EPS[dtype_name], lmi=True,
                                        rho=L.module_for(name).program.rho).to(dtype).cuda()
    for B in L.batches_of(name):
        q = torch.from_numpy(ref.q[:B].copy()).to(dtype).cuda().requires_grad_(True)
        z, iters = layer.project(q)
        (z * torch.from_numpy((ref.gy @ cs.NA_E)[:B]).to(dtype).cuda()).sum().backward()
        assert L.compare(name, dtype_name, z.detach().cpu().numpy(), q.grad.cpu().numpy(), iters.cpu().numpy(), rows=B) == []


def test_strided_input_and_empty_batch():
    name = "k8_eq3_lin5_lmi5"
    pack = _pack(name)
    q, _ = _inputs(name, "float32", 65)
    wide = torch.full((65, q.shape[1] + 3), 7.0, device="cuda")
    wide[:, :q.shape[1]] = q
    z0, it0, _ = ops.proj_forward_raw(q, pack, 200, 1e-6)
    z1, it1, _ = ops.proj_forward_raw(wide, pack, 200, 1e-6)                 # ldq > n
    assert torch.equal(z0, z1) and torch.equal(it0, it1)
    z, iters, vstar = ops.proj_forward_raw(q[:0], pack, 200, 1e-6)
    assert z.shape == (0, pack.n) and iters.shape == (0,) and vstar.shape == (0, pack.m)
    assert ops.proj_backward_raw(q[:0], vstar, iters, pack, 200, 1e-6).shape == (0, pack.n)


@pytest.mark.parametrize("max_iters", [5, 32, 33, 75])
def test_iteration_cap_and_chunk_boundaries(max_iters):
    """Rows that need more than ``max_iters`` end AT the cap and say so, the others are untouched by it: same kernel, same
    arithmetic, so the counts of the uncapped run are met exactly.  33 and 75 are no multiple of the 32 iterations of a
    launch; 32 ends at a launch boundary."""
    name, dtype_name = "r8_k6", "float32"
    pack = _pack(name)
    q, _ = _inputs(name, dtype_name, 65)
    zf, full, _ = ops.proj_forward_raw(q, pack, L.MAX_ITERS, L.EPS[dtype_name])
    z, iters, _ = ops.proj_forward_raw(q, pack, max_iters, L.EPS[dtype_name])
    full, iters = full.cpu().numpy(), iters.cpu().numpy()
    late = full > max_iters
    assert late.any() and (~late).any() and iters.max() == max_iters
    assert np.all(iters[late] == max_iters)
    assert np.array_equal(iters[~late], full[~late]) and torch.equal(z[~late], zf[~late])
    c = L.module_for(name).constants(torch.float32, torch.device("cpu"))
    zm, _, _ = projection.mirror_forward(c, q.cpu(), max_iters, L.EPS[dtype_name])
    assert torch.all(torch.isfinite(z))
    assert np.all(L.row_gap(z.cpu().numpy(), zm.numpy()) <= 1e-4)


def test_a_nan_row_stays_nan_and_alone():
    name = "r3_k4"
    pack = _pack(name)
    q, g = _inputs(name, "float32", 65)
    bad = q.clone()
    bad[17, 1] = float("nan")
    z0, it0, v0 = ops.proj_forward_raw(q, pack, 64, 1e-6)
    z1, it1, v1 = ops.proj_forward_raw(bad, pack, 64, 1e-6)
    keep = torch.arange(65, device="cuda") != 17
    assert torch.all(torch.isnan(z1[17]))
    assert torch.equal(z1[keep], z0[keep]) and torch.equal(it1[keep], it0[keep])
    g0 = ops.proj_backward_raw(g, v0, it0, pack, 64, 1e-6)
    g1 = ops.proj_backward_raw(g, v1, it1, pack, 64, 1e-6)
    assert torch.all(torch.isnan(g1[17])) and torch.equal(g1[keep], g0[keep])


@pytest.mark.eager_detour
def test_r33_refused_warns_matches_the_mirror_and_raises_under_strict(monkeypatch):
    name = L.REFUSED.name
    assert not L.case_served(name, "float32") and not L.case_served(name, "float64")
    cs = L.make_cs(name)
    q = torch.from_numpy(L.make_inputs(name)[0]).float()
    with pytest.raises(_lib.RayenError) as err:              # the raw op never detours
        ops.proj_forward_raw(q.cuda(), _pack(name), 10, 1e-6)
    assert err.value.code == _lib.E_UNSUPPORTED
    layer = projection.ProjectionModule(cs, create_map=False, lmi=True, rho=L.REFUSED.rho, max_iters=300).cuda()
    monkeypatch.setenv("RAYEN_STRICT_HIP", "1")
    with pytest.raises(_lib.RayenError):
        layer.project(q.cuda())
    monkeypatch.setenv("RAYEN_STRICT_HIP", "0")
    with pytest.warns(RuntimeWarning, match="no HIP kernel serves this projection"):
        z, iters = layer.project(q.cuda())
    zm, im = layer.project(q)                                # the mirror on the host
    assert np.all(L.row_gap(z.cpu().numpy(), zm.numpy()) <= 1e-4) and iters.shape == im.shape
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # one warning per module, device and dtype
        layer.project(q.cuda())


def test_up_mode_and_a_linear_mapper():
    name = "k8_eq3_lin5_lmi5"
    cs, ref = L.make_cs(name), L.reference(name)
    rho = L.module_for(name).program.rho
    up = projection.ProjectionModule(cs, create_map=False, mode='UP', lmi=True, rho=rho, max_iters=L.MAX_ITERS).cuda()
    q = torch.from_numpy(ref.q[:65]).float().cuda()
    up.train()
    assert torch.allclose(up(q)[:, :, 0], q @ up.NA_E.T + up.yp.T, rtol=0, atol=1e-6)      # training: the identity
    up.eval()
    z, _ = up.project(q)
    assert np.all(L.row_gap(z.cpu().numpy(), ref.z[:65]) <= L.bars(name, "float32")[0])                # eval: the projection
    assert torch.allclose(up(q)[:, :, 0], z @ up.NA_E.T + up.yp.T, rtol=0, atol=1e-5)
    torch.manual_seed(0)
    net = projection.ProjectionModule(cs, input_dim=6, mode='PP', lmi=True, rho=rho).cuda()
    x = torch.randn(64, 6, device="cuda")
    target = torch.from_numpy(ref.z[:64] @ cs.NA_E.T + cs.yp.T).float().cuda()
    loss = ((net(x)[:, :, 0] - target) ** 2).mean()
    loss.backward()
    grads = [p.grad for p in net.parameters()]
    assert all(g is not None and torch.all(torch.isfinite(g)) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    assert float(np.max(cs.getViolationRows(net(x)[:, :, 0].detach().double().cpu().numpy()))) <= 1e-3
    yb, dist = cs.projectBatch(torch.from_numpy(ref.q[:9] @ cs.NA_E.T + cs.yp.T).float().cuda(), lmi=True)
    assert np.max(np.abs(yb.cpu().numpy() - (ref.z[:9] @ cs.NA_E.T + cs.yp.T))) <= 1e-3 and dist.shape == (9,)
