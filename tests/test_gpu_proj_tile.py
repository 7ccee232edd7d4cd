"""The tile kernel of the Euclidean projection (rayen_amd/csrc/rayen_proj_tile.hip: 32 samples per workgroup on the matrix
cores) through the ops and through ``ProjectionModule(kernel='tile' | 'auto')``, fp32, against the fp64 reference of
tests/proj_reference.py -- for the three cases beyond the wave kernel's envelope from the fixtures of
tests/proj_tile_cases.py.  The bars are the existing ones: KINK_FACTOR times the HOST mirror's gap to the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import proj_reference as pr                                  # noqa: E402
import proj_tile_cases as ptc                                # noqa: E402
from rayen_amd import _lib, ops, projection, workloads       # noqa: E402

pytestmark = pytest.mark.gpu
F32 = "float32"
EPS = pr.EPS[F32]
OLD = [c.name for c in pr.CASES]


def _pack(name):
    return ops.ProjPack(pr.module_for(name).program.arrays(), torch.cuda.current_device())


def _inputs(name, B=pr.BATCH):
    cs = pr.make_cs(name)
    q, gy = pr.make_inputs(name)
    return torch.from_numpy(q[:B]).float().cuda(), torch.from_numpy((gy @ cs.NA_E)[:B]).float().cuda()


def _run(name, B=pr.BATCH, kernel="tile", max_iters=pr.MAX_ITERS):
    pack = _pack(name)
    q, g = _inputs(name, B)
    z, iters, vstar = ops.proj_forward_raw(q, pack, max_iters, EPS, kernel=kernel)
    grad = ops.proj_backward_raw(g, vstar, iters, pack, max_iters, EPS, kernel=kernel)
    return z, iters, vstar, grad


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("name", OLD)
def test_every_existing_case_through_the_tile_kernel(name):
    z, iters, vstar, grad = _run(name)
    run, ref = pr.mirror_run(name, F32), pr.reference(name)
    fwd_bar, _, _ = pr.bars(name, F32)
    zw, _, _ = ops.proj_forward_raw(_inputs(name)[0], _pack(name), pr.MAX_ITERS, EPS)
    print(f"{name}: fwd gap {pr.row_gap(_np(z), ref.z).max():.3e} bwd gap "
          f"{pr.row_gap(_np(grad), ref.grad_q)[~ref.kink].max():.3e} to mirror {pr.row_gap(_np(z), run.z).max():.3e} "
          f"to wave {pr.row_gap(_np(z), _np(zw)).max():.3e} iters max {int(iters.max())} "
          f"(mirror {int(run.iters.max())}) bars {pr.bars(name, F32)}")
    assert pr.compare(name, F32, _np(z), _np(grad), _np(iters)) == []
    assert np.all(pr.row_gap(_np(z), run.z) <= 2 * fwd_bar)
    assert int(iters.max()) < pr.MAX_ITERS
    assert np.all(pr.row_gap(_np(z), _np(zw)) <= 2 * fwd_bar)


@pytest.mark.parametrize("name", ptc.NAMES)
def test_cases_beyond_the_wave_envelope_against_their_fixtures(name):
    assert not pr.served(*ptc.SHAPE[name], 4)
    z, iters, vstar, grad = _run(name)
    ref, run = ptc.reference(name), ptc.mirror_run(name)
    fwd_bar, _, _ = ptc.bars(name)
    print(f"{name}: fwd gap {pr.row_gap(_np(z), ref.z).max():.3e} bwd gap "
          f"{pr.row_gap(_np(grad), ref.grad_q)[~ref.kink].max():.3e} to mirror {pr.row_gap(_np(z), run.z).max():.3e} "
          f"iters max {int(iters.max())} (mirror {int(run.iters.max())}) bars {ptc.bars(name)}")
    assert ptc.compare(name, _np(z), _np(grad), _np(iters)) == []
    assert np.all(pr.row_gap(_np(z), run.z) <= 2 * fwd_bar)
    assert int(iters.max()) < pr.MAX_ITERS


@pytest.mark.parametrize("name", ["k8_n5_ragged_equalities", "n8_mixed_past_576"])
def test_a_rows_arithmetic_does_not_depend_on_its_tile_mates(name):
    full = _run(name)
    for B in (1, 31, 32, 33, 65):
        part = _run(name, B)
        for a, b, what in zip(part, full, ("z", "iters", "vstar", "grad_q")):
            assert torch.equal(a, b[:B]), (B, what)


def test_vstar_and_iters_interchange_with_the_wave_kernel():
    name = "n32_full"
    pack, (q, g) = _pack(name), _inputs(name)
    ok = ~pr.reference(name).kink
    _, bwd_bar, _ = pr.bars(name, F32)
    for fwd, other in (("tile", "wave"), ("wave", "tile")):
        _, iters, vstar = ops.proj_forward_raw(q, pack, pr.MAX_ITERS, EPS, kernel=fwd)
        own = ops.proj_backward_raw(g, vstar, iters, pack, pr.MAX_ITERS, EPS, kernel=fwd)
        crossed = ops.proj_backward_raw(g, vstar, iters, pack, pr.MAX_ITERS, EPS, kernel=other)
        gap = pr.row_gap(_np(crossed), _np(own))[ok]
        print(f"{fwd} forward, {other} backward against {fwd} backward: {gap.max():.3e} (bar {2 * bwd_bar:.3e})")
        assert np.all(gap <= 2 * bwd_bar)


@pytest.mark.parametrize("max_iters", [5, pr.CHUNK, pr.CHUNK + 1, 3 * pr.CHUNK])
def test_iteration_cap_and_chunk_boundaries(max_iters):
    """The assertions of test_gpu_proj.py::test_iteration_cap_and_chunk_boundaries (the tile kernel's chunk is the wave
    kernel's: 32)."""
    name = "n16_four_quadratics"
    pack = _pack(name)
    q, _ = _inputs(name, 65)
    full = pr.mirror_run(name, F32).iters[:65]
    z, iters, _ = ops.proj_forward_raw(q, pack, max_iters, EPS, kernel="tile")
    iters = _np(iters)
    assert iters.max() == max_iters and np.any(full > max_iters)
    late = full > max_iters + 2
    assert np.all(iters[late] == max_iters)
    early = full < max_iters - 2
    assert np.all(np.abs(iters[early] - full[early]) <= 2)
    c = pr.module_for(name).constants(torch.float32, torch.device("cpu"))
    zm, im, _ = projection.mirror_forward(c, q.cpu(), max_iters, EPS)
    assert torch.all(torch.isfinite(z))
    assert np.all(pr.row_gap(_np(z), zm.numpy()) <= 1e-4)


def test_strided_input_and_graph_capture():
    name = "k8_n5_ragged_equalities"
    pack = _pack(name)
    q, _ = _inputs(name, 65)
    wide = torch.full((65, q.shape[1] + 3), 7.0, device="cuda")
    wide[:, :q.shape[1]] = q
    z0, it0, _ = ops.proj_forward_raw(q, pack, 100, 1e-6, kernel="tile")
    z1, it1, _ = ops.proj_forward_raw(wide, pack, 100, 1e-6, kernel="tile")                 # ldq > n
    assert torch.equal(z0, z1) and torch.equal(it0, it1)
    static_q = q.clone()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.proj_forward_raw(static_q, pack, 100, 1e-6, kernel="tile")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            zg, itg, _ = ops.proj_forward_raw(static_q, pack, 100, 1e-6, kernel="tile")
    static_q.copy_(q.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(zg, z0.flip(0)) and torch.equal(itg, it0.flip(0))


def test_a_nan_row_keeps_to_itself():
    name = "n3_box"
    pack = _pack(name)
    q, _ = _inputs(name, 32)
    z0, it0, _ = ops.proj_forward_raw(q, pack, 64, EPS, kernel="tile")
    bad = q.clone()
    bad[13, 1] = float("nan")
    z1, it1, _ = ops.proj_forward_raw(bad, pack, 64, EPS, kernel="tile")
    assert torch.all(torch.isnan(z1[13])) and int(it1[13]) == 64
    keep = torch.arange(32, device="cuda") != 13
    assert torch.equal(z1[keep], z0[keep]) and torch.equal(it1[keep], it0[keep])


def test_refusals_and_defaults():
    assert os.environ.get("RAYEN_STRICT_HIP") == "1"
    name = "n8_rows_past_576"
    pack = _pack(name)
    q, _ = _inputs(name)
    with pytest.raises(_lib.RayenError) as err:                          # fp64 on the tile op
        ops.proj_forward_raw(q.double(), pack, 10, 1e-9, kernel="tile")
    assert err.value.code == _lib.E_UNSUPPORTED
    import proj_lmi_reference as plr
    lmi_module = plr.module_for("r3_k4")
    lmi_pack = ops.ProjPack(lmi_module.program.arrays(), torch.cuda.current_device())
    ql = torch.zeros((4, lmi_pack.n), device="cuda")
    assert not ops.proj_tile_served(lmi_pack)
    with pytest.raises(_lib.RayenError) as err:                          # a PSD block
        ops.proj_forward_raw(ql, lmi_pack, 10, 1e-6, kernel="tile")
    assert err.value.code == _lib.E_UNSUPPORTED
    cs = pr.make_cs(name)
    default = projection.ProjectionModule(cs, create_map=False).cuda()
    assert default.kernel == "wave"
    with pytest.raises(_lib.RayenError):                                 # the default kernel still refuses the set
        default.project(q)
    ref = ptc.reference(name)
    g = torch.from_numpy(ref.gy @ cs.NA_E).float().cuda()
    for kernel in ("auto", "tile"):
        layer = projection.ProjectionModule(cs, create_map=False, max_iters=pr.MAX_ITERS, eps=EPS, kernel=kernel).cuda()
        leaf = q.clone().requires_grad_(True)
        z, iters = layer.project(leaf)
        (z * g).sum().backward()
        assert ptc.compare(name, _np(z), _np(leaf.grad), _np(iters)) == []
    yb, dist = cs.projectBatch(q @ torch.from_numpy(cs.NA_E.T).float().cuda() + torch.from_numpy(cs.yp.T).float().cuda(),
                               kernel="tile")
    fwd_bar, _, _ = ptc.bars(name)
    want = ref.z @ cs.NA_E.T + cs.yp.T
    assert np.all(pr.row_gap(_np(yb), want) <= fwd_bar) and dist.shape == (pr.BATCH,)


def test_module_on_the_tile_kernel_trains():
    name = "n6_forty_cones"
    cs, ref = pr.make_cs(name), ptc.reference(name)
    torch.manual_seed(0)
    net = projection.ProjectionModule(cs, input_dim=6, mode='PP', kernel='tile').cuda()
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


# The two largest instances (12 blocks a wave at n <= 32, 10 at n > 32): the only ones that keep p of their last blocks in
# LDS, and the ones config 5 runs.  No fp64 reference here (config 5's takes minutes on the host): the mirror on the device
# runs the same iteration to the same cap, so the two differ by summation order only; the bar is the 1e-4 that
# test_iteration_cap_and_chunk_boundaries holds a capped run to.
LARGE = {"c5_twelve_blocks": (lambda: workloads.make_raw("c5"), 0.9, 12),
         "n40_nine_blocks": (lambda: workloads.random_lin_quad_soc(40, 900, 2, 1, seed=21), 0.5, 9)}


@pytest.mark.parametrize("name", list(LARGE))
def test_the_largest_instances_against_the_mirror_on_the_device(name):
    import tile_layout_formulas as tl
    make, amp, blocks = LARGE[name]
    cs = workloads.build_constraints(make())
    layer = projection.ProjectionModule(cs, create_map=False, rho=1.0)
    prog = layer.program
    assert tl.layout(prog.m_lin, prog.soc_rows)[3] == blocks and blocks > 6          # (beyond the 6-block instances)
    pack = ops.ProjPack(prog.arrays(), torch.cuda.current_device())
    assert ops.proj_tile_served(pack) and not ops.proj_wave_served(pack, torch.float32)
    B, max_iters = 33, 40                                                            # two launches: 32 + 8 iterations
    rng = np.random.default_rng(len(name))
    q = cs.z0.reshape(1, -1) + amp * rng.uniform(0.0, 1.5, (B, 1)) * rng.standard_normal((B, cs.n))
    q = torch.from_numpy(q).float().cuda()
    g = torch.from_numpy(rng.standard_normal((B, cs.n))).float().cuda()
    with pytest.raises(_lib.RayenError) as err:
        ops.proj_forward_raw(q, pack, max_iters, EPS)
    assert err.value.code == _lib.E_UNSUPPORTED
    z, iters, vstar = ops.proj_forward_raw(q, pack, max_iters, EPS, kernel="tile")
    grad = ops.proj_backward_raw(g, vstar, iters, pack, max_iters, EPS, kernel="tile")
    c = layer.constants(torch.float32, q.device)
    zm, im, vm = projection.mirror_forward(c, q, max_iters, EPS)
    gm = projection.mirror_backward(c, g, vstar, iters, max_iters, EPS)              # (at the kernel's own v*)
    im, it = _np(im), _np(iters)
    print(f"{name}: n={prog.n} m={prog.m} cones={len(prog.soc_rows)}; iters tile max {it.max()} mean {it.mean():.1f}, mirror "
          f"max {im.max()}; z gap {pr.row_gap(_np(z), _np(zm)).max():.3e} v* gap {pr.row_gap(_np(vstar), _np(vm)).max():.3e} "
          f"grad gap {pr.row_gap(_np(grad), _np(gm)).max():.3e}")
    assert it.max() == max_iters and np.any(it < max_iters)                          # rows at the cap, and rows that are not
    assert np.array_equal(it == 0, im == 0)
    assert np.all(np.abs(it - im)[im < max_iters - 2] <= 2) and np.all(it[im == max_iters] >= max_iters - 2)
    assert torch.all(torch.isfinite(z)) and torch.all(torch.isfinite(grad))
    assert np.all(pr.row_gap(_np(z), _np(zm)) <= 1e-4)
    assert np.all(pr.row_gap(_np(vstar), _np(vm)) <= 1e-4)
    assert np.all(pr.row_gap(_np(grad), _np(gm)) <= 1e-4)
    assert torch.equal(z[iters == 0], q[iters == 0])
