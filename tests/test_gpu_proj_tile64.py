"""The fp64 tile kernel of the Euclidean projection (rayen_amd/csrc/rayen_proj_tile64.hip: 16 samples per workgroup on the
fp64 matrix cores) through the ops and through ``ProjectionModule(kernel='tile' | 'auto')`` on fp64 input, against the fp64
reference of tests/proj_reference.py: every case of that module, the boundary cases of tests/proj_sweep_cases.py and the
three cases of tests/proj_tile_cases.py.  The bars are the existing ones at fp64: KINK_FACTOR times the HOST mirror's gap to
the reference, never the kernel's own (tests/proj_tile64_cases.py feeds them from the fixtures)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import proj_reference as pr                                  # noqa: E402
import proj_sweep_cases as psc                               # noqa: E402
import proj_tile_cases as ptc                                # noqa: E402
import proj_tile64_cases as p64                              # noqa: E402
from rayen_amd import _lib, ops, projection, workloads       # noqa: E402

pytestmark = pytest.mark.gpu
F64 = "float64"
EPS = pr.EPS[F64]
OLD = [c.name for c in pr.CASES]
UNCAPPED = {"n64_c3_shape"}          # the capped 1e-6 bar is below the fp64 HOST mirror's own backward gap (1.1e-6) there
# what only the order of the sums separates: the 1e-4 the fp32 tests hold a capped run to (test_gpu_proj_tile.py), scaled by
# the ratio of the machine epsilons, times 16 for the longer fp64 sums (about 3e-12)
ORDER_BAR = 1e-4 * (np.finfo(np.float64).eps / np.finfo(np.float32).eps) * 16.0


def _pack(name):
    return ops.ProjPack(pr.module_for(name).program.arrays(), torch.cuda.current_device())


def _inputs(name, B=None):
    cs = pr.make_cs(name)
    q, gy = pr.make_inputs(name)
    B = p64.rows_of(name) if B is None else B
    return torch.from_numpy(q[:B]).cuda(), torch.from_numpy((gy @ cs.NA_E)[:B]).cuda()


def _run(name, B=None, kernel="tile64", max_iters=pr.MAX_ITERS):
    pack = _pack(name)
    q, g = _inputs(name, B)
    z, iters, vstar = ops.proj_forward_raw(q, pack, max_iters, EPS, kernel=kernel)
    grad = ops.proj_backward_raw(g, vstar, iters, pack, max_iters, EPS, kernel=kernel)
    return z, iters, vstar, grad


def _np(t):
    return t.detach().cpu().numpy()


def _judge(name, z, iters, grad):
    capped = name not in UNCAPPED
    ref, run = p64.reference(name), p64.host_mirror(name)
    fwd_bar, bwd_bar, _ = p64.bars(name, capped)
    ok = ~ref.kink
    print(f"{name}: fwd gap {pr.row_gap(_np(z), ref.z).max():.3e} bwd gap {pr.row_gap(_np(grad), ref.grad_q)[ok].max():.3e} "
          f"to mirror {pr.row_gap(_np(z), run.z).max():.3e} iters max {int(iters.max())} mean {float(iters.float().mean()):.1f} "
          f"(mirror {int(run.iters.max())}) kink rows {int(np.count_nonzero(ref.kink))} bars {p64.bars(name, capped)}")
    assert p64.compare(name, _np(z), _np(grad), _np(iters), capped=capped) == []
    assert np.all(pr.row_gap(_np(z), run.z) <= 2 * fwd_bar)
    assert int(iters.max()) < pr.MAX_ITERS
    return fwd_bar, bwd_bar


@pytest.mark.parametrize("name", OLD)
def test_every_existing_case_in_fp64(name):
    z, iters, vstar, grad = _run(name)
    fwd_bar, _ = _judge(name, z, iters, grad)
    if pr.case_served(name, F64):
        zw, _, _ = ops.proj_forward_raw(_inputs(name)[0], _pack(name), pr.MAX_ITERS, EPS)
        print(f"{name}: to wave {pr.row_gap(_np(z), _np(zw)).max():.3e}")
        assert np.all(pr.row_gap(_np(z), _np(zw)) <= 2 * fwd_bar)
    else:
        assert name == "n64_c3_shape" and not ops.proj_wave_served(_pack(name), torch.float64)
        assert np.count_nonzero(p64.reference(name).kink) <= pr.kink_cap(pr.BATCH)


@pytest.mark.parametrize("name", p64.SWEEP_WAVE + p64.SWEEP_BEYOND)
def test_the_boundary_cases_in_fp64(name):
    assert (name in p64.SWEEP_WAVE) == ops.proj_wave_served(_pack(name), torch.float64)
    z, iters, vstar, grad = _run(name)
    _judge(name, z, iters, grad)


@pytest.mark.parametrize("name", ptc.NAMES)
def test_cases_beyond_the_wave_envelope_in_fp64(name):
    pack = _pack(name)
    assert not ops.proj_wave_served(pack, torch.float64)
    assert ops.proj_tile64_served(pack)
    z, iters, vstar, grad = _run(name)
    _judge(name, z, iters, grad)


@pytest.mark.parametrize("name", ["k8_n5_ragged_equalities", "n8_mixed_past_576"])
def test_a_rows_bits_do_not_depend_on_its_tile_mates(name):
    full = _run(name, 65)
    for B in (1, 15, 16, 17, 33):
        part = _run(name, B)
        for a, b, what in zip(part, full, ("z", "iters", "vstar", "grad_q")):
            assert torch.equal(a, b[:B]), (B, what)


def test_vstar_and_iters_interchange_with_the_wave_kernel():
    name = "n32_full"
    pack, (q, g) = _pack(name), _inputs(name)
    ok = ~pr.reference(name).kink
    _, bwd_bar, _ = pr.bars(name, F64)
    for fwd, other in (("tile64", "wave"), ("wave", "tile64")):
        _, iters, vstar = ops.proj_forward_raw(q, pack, pr.MAX_ITERS, EPS, kernel=fwd)
        own = ops.proj_backward_raw(g, vstar, iters, pack, pr.MAX_ITERS, EPS, kernel=fwd)
        crossed = ops.proj_backward_raw(g, vstar, iters, pack, pr.MAX_ITERS, EPS, kernel=other)
        gap = pr.row_gap(_np(crossed), _np(own))[ok]
        print(f"{fwd} forward, {other} backward against {fwd} backward: {gap.max():.3e} (bar {2 * bwd_bar:.3e})")
        assert np.all(gap <= 2 * bwd_bar)


@pytest.mark.parametrize("max_iters", [5, pr.CHUNK, pr.CHUNK + 1, 3 * pr.CHUNK])
def test_iteration_cap_and_chunk_boundaries(max_iters):
    """The assertions of test_gpu_proj.py::test_iteration_cap_and_chunk_boundaries in fp64.  Against the mirror on the same
    inputs to the same cap: a row that took the mirror's number of iterations differs from it by the order of the sums
    (ORDER_BAR); a row that met the stop rule an iteration apart differs by a step of a converged iteration, which the
    stop rule itself bounds by eps (1 + max|xt|) -- 4 eps with the project's factor."""
    name = "n16_four_quadratics"
    pack = _pack(name)
    q, _ = _inputs(name, 65)
    full = pr.mirror_run(name, F64).iters[:65]
    z, iters, _ = ops.proj_forward_raw(q, pack, max_iters, EPS, kernel="tile64")
    iters = _np(iters)
    assert iters.max() == max_iters and np.any(full > max_iters)
    late = full > max_iters + 2
    assert np.all(iters[late] == max_iters)
    early = full < max_iters - 2
    assert np.all(np.abs(iters[early] - full[early]) <= 2)
    c = pr.module_for(name).constants(torch.float64, torch.device("cpu"))
    zm, im, _ = projection.mirror_forward(c, q.cpu(), max_iters, EPS)
    gap, agree = pr.row_gap(_np(z), zm.numpy()), iters == im.numpy()
    print(f"max_iters {max_iters}: rows with the mirror's count {int(agree.sum())} of 65, gap {gap[agree].max():.3e} "
          f"(bar {ORDER_BAR:.3e}); the others {gap[~agree].max() if (~agree).any() else 0.0:.3e} (bar {pr.KINK_FACTOR * EPS:.1e})")
    assert torch.all(torch.isfinite(z))
    assert np.all(gap[agree] <= ORDER_BAR) and np.all(gap[~agree] <= pr.KINK_FACTOR * EPS)


def test_strided_input_and_graph_capture():
    name = "k8_n5_ragged_equalities"
    pack = _pack(name)
    q, g = _inputs(name, 65)
    wide = torch.full((65, q.shape[1] + 3), 7.0, device="cuda", dtype=torch.float64)
    wide[:, :q.shape[1]] = q
    wide_g = torch.full((65, q.shape[1] + 5), -3.0, device="cuda", dtype=torch.float64)
    wide_g[:, :q.shape[1]] = g
    z0, it0, v0 = ops.proj_forward_raw(q, pack, 100, EPS, kernel="tile64")
    z1, it1, v1 = ops.proj_forward_raw(wide, pack, 100, EPS, kernel="tile64")                # ldq > n
    assert torch.equal(z0, z1) and torch.equal(it0, it1) and torch.equal(v0, v1)
    g0 = ops.proj_backward_raw(g, v0, it0, pack, 100, EPS, kernel="tile64")
    g1 = ops.proj_backward_raw(wide_g, v0, it0, pack, 100, EPS, kernel="tile64")             # ldg > n
    assert torch.equal(g0, g1)
    static_q = q.clone()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.proj_forward_raw(static_q, pack, 100, EPS, kernel="tile64")                      # (the warm call: the upload)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            zg, itg, _ = ops.proj_forward_raw(static_q, pack, 100, EPS, kernel="tile64")
    static_q.copy_(q.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(zg, z0.flip(0)) and torch.equal(itg, it0.flip(0))


def test_a_nan_row_keeps_to_itself():
    name = "n3_box"
    pack = _pack(name)
    q, _ = _inputs(name, 32)
    z0, it0, _ = ops.proj_forward_raw(q, pack, 64, EPS, kernel="tile64")
    bad = q.clone()
    bad[13, 1] = float("nan")
    z1, it1, _ = ops.proj_forward_raw(bad, pack, 64, EPS, kernel="tile64")
    assert torch.all(torch.isnan(z1[13])) and int(it1[13]) == 64
    keep = torch.arange(32, device="cuda") != 13
    assert torch.equal(z1[keep], z0[keep]) and torch.equal(it1[keep], it0[keep])


def test_the_largest_instance_against_the_mirror_on_the_device():
    """Config 5's program on the (24, 2) instance, the one that keeps p of its last six blocks in LDS.  The mirror on the
    device runs the same iteration to the same cap: the two differ by the order of the sums only (ORDER_BAR)."""
    import tile64_layout_formulas as tl
    cs = workloads.build_constraints(workloads.make_raw("c5"))
    layer = projection.ProjectionModule(cs, create_map=False, rho=1.0)
    prog = layer.program
    assert (prog.n, prog.m, len(prog.soc_rows)) == (30, 1410, 72)
    assert tl.instance(tl.layout(prog.m_lin, prog.soc_rows)[3], prog.n) == (24, 2)
    pack = ops.ProjPack(prog.arrays(), torch.cuda.current_device())
    assert ops.proj_tile64_served(pack) and not ops.proj_wave_served(pack, torch.float64)
    B, max_iters = 17, 40                                                            # two launches: 32 + 8 iterations
    rng = np.random.default_rng(5)
    q = cs.z0.reshape(1, -1) + 0.9 * rng.uniform(0.0, 1.5, (B, 1)) * rng.standard_normal((B, cs.n))
    q = torch.from_numpy(q).cuda()
    g = torch.from_numpy(rng.standard_normal((B, cs.n))).cuda()
    with pytest.raises(_lib.RayenError) as err:
        ops.proj_forward_raw(q, pack, max_iters, EPS)
    assert err.value.code == _lib.E_UNSUPPORTED
    z, iters, vstar = ops.proj_forward_raw(q, pack, max_iters, EPS, kernel="tile64")
    grad = ops.proj_backward_raw(g, vstar, iters, pack, max_iters, EPS, kernel="tile64")
    c = layer.constants(torch.float64, q.device)
    zm, im, vm = projection.mirror_forward(c, q, max_iters, EPS)
    gm = projection.mirror_backward(c, g, vstar, iters, max_iters, EPS)              # (at the kernel's own v*)
    im, it = _np(im), _np(iters)
    print(f"c5: n={prog.n} m={prog.m} cones={len(prog.soc_rows)}; iters tile64 max {it.max()} mean {it.mean():.1f}, mirror "
          f"max {im.max()}; z gap {pr.row_gap(_np(z), _np(zm)).max():.3e} v* gap {pr.row_gap(_np(vstar), _np(vm)).max():.3e} "
          f"grad gap {pr.row_gap(_np(grad), _np(gm)).max():.3e} (bar {ORDER_BAR:.3e})")
    assert it.max() == max_iters and np.any(it < max_iters)                          # rows at the cap, and rows that are not
    assert np.array_equal(it == 0, im == 0)
    assert np.all(np.abs(it - im)[im < max_iters - 2] <= 2) and np.all(it[im == max_iters] >= max_iters - 2)
    assert torch.all(torch.isfinite(z)) and torch.all(torch.isfinite(grad))
    assert np.all(pr.row_gap(_np(z), _np(zm)) <= ORDER_BAR)
    assert np.all(pr.row_gap(_np(vstar), _np(vm)) <= ORDER_BAR)
    assert np.all(pr.row_gap(_np(grad), _np(gm)) <= ORDER_BAR)
    assert torch.equal(z[iters == 0], q[iters == 0])


def test_the_raw_ops_accept_tile64():
    """On the parent commit ``kernel="tile64"`` is a ValueError."""
    name = "n64_c3_shape"
    pack = _pack(name)
    q, g = _inputs(name, 33)
    assert ops.PROJ_KERNELS == ("wave", "tile") and ops.PROJ_KERNELS_F64 == ("wave", "tile64")
    z, iters, vstar = ops.proj_forward_raw(q, pack, pr.MAX_ITERS, EPS, kernel="tile64")
    grad = ops.proj_backward_raw(g, vstar, iters, pack, pr.MAX_ITERS, EPS, kernel="tile64")
    assert z.dtype == grad.dtype == vstar.dtype == torch.float64 and iters.dtype == torch.int32
    assert pr.compare(name, F64, _np(z), _np(grad), _np(iters), rows=33, capped=False) == []
    with pytest.raises(ValueError):
        ops.proj_forward_raw(q, pack, 10, EPS, kernel="tile65")


@pytest.mark.parametrize("kernel", ["tile", "auto"])
def test_the_module_serves_config_3_in_fp64(kernel):
    """On the parent commit both raise under RAYEN_STRICT_HIP=1: no fp64 kernel held n64_c3_shape."""
    assert os.environ.get("RAYEN_STRICT_HIP") == "1"
    name = "n64_c3_shape"
    cs, ref = pr.make_cs(name), pr.reference(name)
    q, g = _inputs(name)
    layer = projection.ProjectionModule(cs, create_map=False, max_iters=pr.MAX_ITERS, eps=EPS, kernel=kernel).double().cuda()
    leaf = q.clone().requires_grad_(True)
    z, iters = layer.project(leaf)
    (z * g).sum().backward()
    assert z.dtype == torch.float64
    assert pr.compare(name, F64, _np(z), _np(leaf.grad), _np(iters), capped=False) == []
    # fp32 input on the same module: the fp32 kernels, as before
    z32, it32 = layer.project(q.float())
    assert z32.dtype == torch.float32 and pr.compare(name, "float32", _np(z32), _np(leaf.grad), _np(it32), backward=False) == []


def test_project_batch_in_fp64_on_the_tile_kernel():
    name = "n8_rows_past_576"
    cs, ref = pr.make_cs(name), p64.reference(name)
    q, _ = _inputs(name)
    Y = q @ torch.from_numpy(cs.NA_E.T).cuda() + torch.from_numpy(cs.yp.T).cuda()
    yb, dist = cs.projectBatch(Y, max_iters=pr.MAX_ITERS, eps=EPS, kernel="tile")
    fwd_bar, _, _ = p64.bars(name)
    want = ref.z @ cs.NA_E.T + cs.yp.T
    assert yb.dtype == torch.float64 and dist.shape == (pr.BATCH,)
    assert np.all(pr.row_gap(_np(yb), want) <= fwd_bar)
    with pytest.raises(_lib.RayenError):                                 # the default kernel still refuses the set
        cs.projectBatch(Y, max_iters=pr.MAX_ITERS, eps=EPS)


def test_module_on_the_fp64_tile_kernel_trains():
    name = "n6_forty_cones"
    cs, ref = pr.make_cs(name), p64.reference(name)
    torch.manual_seed(0)
    net = projection.ProjectionModule(cs, input_dim=6, mode='PP', kernel='tile', max_iters=pr.MAX_ITERS, eps=EPS).double().cuda()
    assert not ops.proj_wave_served(net.proj_pack(torch.device("cuda", torch.cuda.current_device()))[0], torch.float64)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    x = torch.randn(64, 6, device="cuda", dtype=torch.float64)
    target = torch.from_numpy(ref.z[:64] @ cs.NA_E.T + cs.yp.T).cuda()
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = ((net(x)[:, :, 0] - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"losses {losses} iters max {int(net.proj_iters.max())}")
    assert losses[-1] < losses[0] and np.isfinite(losses).all()
    assert float(np.max(cs.getViolationRows(_np(net(x)[:, :, 0])))) <= 1e-6


def test_refusals_stay():
    assert os.environ.get("RAYEN_STRICT_HIP") == "1"
    name = "n8_rows_past_576"
    pack = _pack(name)
    q, _ = _inputs(name, 33)
    with pytest.raises(_lib.RayenError) as err:                          # fp32 on the fp64 tile op
        ops.proj_forward_raw(q.float(), pack, 10, 1e-6, kernel="tile64")
    assert err.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(_lib.RayenError) as err:                          # fp64 on the fp32 tile op, as before
        ops.proj_forward_raw(q, pack, 10, EPS, kernel="tile")
    assert err.value.code == _lib.E_UNSUPPORTED
    import proj_lmi_reference as plr
    lmi_pack = ops.ProjPack(plr.module_for("r3_k4").program.arrays(), torch.cuda.current_device())
    assert not ops.proj_tile64_served(lmi_pack)
    with pytest.raises(_lib.RayenError) as err:                          # a PSD block
        ops.proj_forward_raw(torch.zeros((4, lmi_pack.n), device="cuda", dtype=torch.float64), lmi_pack, 10, EPS, kernel="tile64")
    assert err.value.code == _lib.E_UNSUPPORTED
    import tile64_layout_formulas as tl
    for n, rows in ((8, tl.MAX_ROWS + 1), (65, 40)):                     # one row past the largest layout; n = 65
        rng = np.random.default_rng(rows)
        G = rng.standard_normal((rows, n))
        prog = projection.Program(G, np.ones(rows), rows, [], n, 1.0)
        big = ops.ProjPack(prog.arrays(), torch.cuda.current_device())
        assert not ops.proj_tile64_served(big)
        with pytest.raises(_lib.RayenError) as err:
            ops.proj_forward_raw(torch.zeros((4, n), device="cuda", dtype=torch.float64), big, 10, EPS, kernel="tile64")
        assert err.value.code == _lib.E_UNSUPPORTED
    largest = projection.Program(np.random.default_rng(1).standard_normal((tl.MAX_ROWS, 8)), np.ones(tl.MAX_ROWS), tl.MAX_ROWS, [], 8, 1.0)
    assert ops.proj_tile64_served(ops.ProjPack(largest.arrays(), torch.cuda.current_device()))
    c3 = "n64_c3_shape"
    default = projection.ProjectionModule(pr.make_cs(c3), create_map=False).double().cuda()
    assert default.kernel == "wave"
    with pytest.raises(_lib.RayenError):                                 # the default kernel still refuses config 3 in fp64
        default.project(_inputs(c3, 17)[0])
