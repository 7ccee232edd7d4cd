"""The Euclidean-projection kernels (rayen_amd/csrc/rayen_proj.hip: wave per sample, fp32 and fp64;
rayen_amd/csrc/rayen_proj_tile.hip: tiles of 32 samples, fp32) at their boundaries, against the fp64 reference of
tests/proj_reference.py from the fixtures of tests/proj_sweep_cases.py: every register-count instantiation and every tile
instance at its edges, the wave kernel's grid-stride loop and both passes of its leave-early scan, whole-tile states of the
tile kernel, the edges of the backward's scaling, and the refusals.  The bars are the existing ones (``pr.bars``: KINK_FACTOR
times the HOST mirror's gap to the reference); where a test says bit-equal it is because a row's arithmetic depends neither
on the batch size nor on the row's position."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import proj_lmi_reference as plr                             # noqa: E402
import proj_reference as pr                                  # noqa: E402
import proj_sweep_cases as sw                                # noqa: E402
from rayen_amd import _lib, ops, projection, workloads       # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = sw.F32, sw.F64
WHAT = ("z", "iters", "vstar", "grad_q")


def _np(t):
    return t.detach().cpu().numpy()


def _family(name):
    """``(module, (q, gy), seeded rows, max_iters, eps by precision)`` of a case of any of the three case tables."""
    if name in plr.CASE:
        return plr.module_for(name), plr.make_inputs(name), plr.CASE[name].batch, plr.MAX_ITERS, plr.EPS
    rows = sw.BATCH if name in sw.BY_NAME else pr.BATCH
    return pr.module_for(name), pr.make_inputs(name, rows), rows, pr.MAX_ITERS, pr.EPS


_PACKS = {}


def _pack(name):
    if name not in _PACKS:
        _PACKS[name] = ops.ProjPack(_family(name)[0].program.arrays(), torch.cuda.current_device())
    return _PACKS[name]


def _inputs(name, dtype_name, index=None):
    """``(q, g)`` on the device: the seeded rows, or those ``index`` picks."""
    module, (q, gy), rows, _, _ = _family(name)
    cs = plr.make_cs(name) if name in plr.CASE else pr.make_cs(name)
    index = np.arange(rows) if index is None else index
    dtype = getattr(torch, dtype_name)
    return torch.from_numpy(q[index]).to(dtype).cuda(), torch.from_numpy((gy @ cs.NA_E)[index]).to(dtype).cuda()


def _run(name, dtype_name, kernel="wave", index=None, q=None, g=None):
    """``(z, iters, vstar, grad_q)`` of the ops."""
    _, _, _, max_iters, eps = _family(name)
    pack = _pack(name)
    if q is None:
        q, g = _inputs(name, dtype_name, index)
    z, iters, vstar = ops.proj_forward_raw(q, pack, max_iters, eps[dtype_name], kernel=kernel)
    grad = ops.proj_backward_raw(g, vstar, iters, pack, max_iters, eps[dtype_name], kernel=kernel)
    return z, iters, vstar, grad


_SEEDED = {}


def _seeded(name, dtype_name, kernel="wave"):
    """The run on the seeded batch, once."""
    key = (name, dtype_name, kernel)
    if key not in _SEEDED:
        _SEEDED[key] = _run(name, dtype_name, kernel)
    return _SEEDED[key]


def _assert_twins(big, small, index, label):
    """Every row of ``big`` is bit for bit row ``index[b]`` of ``small`` (NaN == NaN)."""
    at = torch.from_numpy(np.asarray(index)).cuda()
    for a, b, what in zip(big, small, WHAT):
        want = b[at]
        same = (a == want) | ((a != a) & (want != want))
        assert bool(same.all()), (label, what, int((~same).reshape(len(at), -1).any(1).sum()), "rows differ")


# ------------------------------------------------------------------ 1. every sweep case against its fixture
RUNS = ([(name, dtype_name, "wave") for name, dtype_name in sw.WAVE_RUNS] + [(name, F32, "tile") for name in sw.NAMES])


@pytest.mark.parametrize("name,dtype_name,kernel", RUNS)
def test_sweep_case_against_its_fixture(name, dtype_name, kernel):
    case = sw.BY_NAME[name]
    pack = _pack(name)
    assert ops.proj_tile_served(pack)
    assert ops.proj_wave_served(pack, getattr(torch, dtype_name)) == (case.R is not None)
    z, iters, vstar, grad = _seeded(name, dtype_name, kernel)
    ref, run = sw.reference(name), sw.mirror_run(name, dtype_name)
    fwd_bar, bwd_bar, _ = sw.bars(name, dtype_name)
    print(f"{name} {dtype_name} {kernel}: fwd gap {pr.row_gap(_np(z), ref.z).max():.3e} bwd gap "
          f"{pr.row_gap(_np(grad), ref.grad_q)[~ref.kink].max():.3e} to mirror {pr.row_gap(_np(z), run.z).max():.3e} "
          f"iters max {int(iters.max())} mean {float(iters.float().mean()):.1f} (mirror {int(run.iters.max())}) "
          f"bars {sw.bars(name, dtype_name)}")
    assert sw.compare(name, dtype_name, _np(z), _np(grad), _np(iters)) == []
    assert np.all(pr.row_gap(_np(z), run.z) <= 2 * fwd_bar)
    assert int(iters.max()) < pr.MAX_ITERS
    if kernel == "tile" and case.R is not None:
        zw = _seeded(name, F32, "wave")[0]
        print(f"{name}: tile to wave {pr.row_gap(_np(z), _np(zw)).max():.3e}")
        assert np.all(pr.row_gap(_np(z), _np(zw)) <= 2 * fwd_bar)


@pytest.mark.parametrize("dtype_name", [F32, F64])
def test_a_psd_block_at_three_rows_a_lane(dtype_name):
    """``proj_kernel<T, 3, *, true>``: r = 12, 78 rows.  The assertions of tests/test_gpu_proj_lmi.py."""
    name = sw.LMI_R3
    z, iters, vstar, grad = _seeded(name, dtype_name)
    ref, run = plr.reference(name), plr.mirror_run(name, dtype_name)
    fwd_bar = plr.bars(name, dtype_name)[0]
    print(f"{name} {dtype_name}: fwd gap {plr.row_gap(_np(z), ref.z).max():.3e} bwd gap "
          f"{plr.row_gap(_np(grad), ref.grad_q)[~ref.kink].max():.3e} to mirror {plr.row_gap(_np(z), run.z).max():.3e} "
          f"iters max {int(iters.max())} mean {float(iters.float().mean()):.1f} (mirror {int(run.iters.max())}) "
          f"bars {plr.bars(name, dtype_name)}")
    assert plr.compare(name, dtype_name, _np(z), _np(grad), _np(iters)) == []
    assert np.all(plr.row_gap(_np(z), run.z) <= 2 * fwd_bar)
    assert int(iters.max()) < plr.MAX_ITERS


# ------------------------------------------------------------------ 2. batch stride, wave kernel
def _shape4(name):
    if name in plr.CASE:
        n, m, _, r = plr.SHAPE[name]
        return n, m, r
    n, m, _ = sw.SHAPE[name] if name in sw.SHAPE else pr.SHAPE[name]
    return n, m, 0


def _compare(name, dtype_name, z, grad, iters, rows=None):
    if name in plr.CASE:
        if name == sw.LMI_STRIDE:
            sw.install_lmi()                                     # (its reference and fp64 mirror from the fixture)
        return plr.compare(name, dtype_name, z, grad, iters, rows=rows)
    if name in sw.BY_NAME:
        return sw.compare(name, dtype_name, z, grad, iters, rows=rows)
    return pr.compare(name, dtype_name, z, grad, iters, rows=rows)


# case, precision, workgroups per CU the grid cap assumes, batch: workgroup 0 owns three whole groups and the batch ends on a
# ragged one (r32_k4, 143 KiB and a Jacobi sweep per iteration: two groups, just past 1 024 rows; 2 s a run of that batch on
# the MI355X; its reference and fp64 mirror, 12 s on the host, come from a fixture)
STRIDE = [("n64_c3_shape", F32, 1, sw.stride_batch(256)), ("m576", F64, 2, sw.stride_batch(512)), ("r32_k4", F64, 1, 1029)]


@pytest.mark.parametrize("name,dtype_name,per_cu,B", STRIDE, ids=[s[0] for s in STRIDE])
def test_a_workgroup_strides_over_several_groups(name, dtype_name, per_cu, B):
    n, m, r = _shape4(name)
    geometry = sw.wave_grid(n, m, r, 4 if dtype_name == F32 else 8, B)
    assert geometry.per_cu == per_cu and geometry.grid == 256 * per_cu and geometry.per_workgroup >= 2 and B % 4 == 1
    rows = _family(name)[2]
    small = _seeded(name, dtype_name)
    assert _compare(name, dtype_name, _np(small[0]), _np(small[3]), _np(small[1])) == []
    # whole copies of the seeded batch, each in its own permutation, then its leading rows
    index = sw.tiled_index(rows, B)
    start = time.perf_counter()
    big = _run(name, dtype_name, index=index)
    torch.cuda.synchronize()
    print(f"{name} {dtype_name} B={B}: grid {geometry.grid}, {geometry.per_workgroup} groups a workgroup, "
          f"{time.perf_counter() - start:.2f} s forward + backward")
    _assert_twins(big, small, index, "tiled")
    z, iters, _, grad = (_np(t) for t in big)
    copies, tail = divmod(B, rows)
    for k in range(copies):
        back = np.argsort(index[rows * k:rows * (k + 1)]) + rows * k
        assert _compare(name, dtype_name, z[back], grad[back], iters[back]) == [], k
    if tail:
        assert _compare(name, dtype_name, z[-tail:], grad[-tail:], iters[-tail:], rows=tail) == []
    # whole groups interior, whole groups finished in the first launch, live rows between finished ones
    index = sw.grouped_index(_np(small[1]), B)
    _assert_twins(_run(name, dtype_name, index=index), small, index, "grouped")


# ------------------------------------------------------------------ 3. the leave-early scan's second pass
# n3_box in fp64 (in fp32 none of its rows needs a second launch, so no scan runs: there k8_n5_ragged_equalities, whose
# image also fits eight times a CU and whose rows take up to 49 iterations)
SCAN = [("n3_box", F64), ("k8_n5_ragged_equalities", F32)]


@pytest.mark.parametrize("name,dtype_name", SCAN)
def test_the_leave_early_scan_takes_a_second_pass(name, dtype_name):
    """524 293 rows: 131 074 groups on 2 048 workgroups, so a workgroup's scan covers 64 groups in its first pass and one
    more in its second.  The box's reference is the clip, exact (test_box_is_clip)."""
    B = sw.SCAN_BATCH
    n, m, _ = pr.SHAPE[name]
    geometry = sw.wave_grid(n, m, 0, 4 if dtype_name == F32 else 8, B)
    assert geometry.scan_passes == 2 and geometry.per_workgroup == 65 and geometry.grid == 2048
    small = _seeded(name, dtype_name)
    assert pr.compare(name, dtype_name, _np(small[0]), _np(small[3]), _np(small[1])) == []
    assert int(small[1].max()) > pr.CHUNK                        # (later launches exist: the scan runs)
    index = np.concatenate((np.arange(pr.BATCH), sw.tiled_index(pr.BATCH, B - pr.BATCH)))
    start = time.perf_counter()
    big = _run(name, dtype_name, index=index)
    torch.cuda.synchronize()
    print(f"{name} {dtype_name} B={B}: {time.perf_counter() - start:.2f} s forward + backward, iters max {int(big[1].max())}")
    if name == "n3_box":
        q = pr.make_inputs(name)[0][index]
        fwd_bar, _, _ = pr.bars(name, dtype_name)
        gap = pr.row_gap(_np(big[0]), np.clip(q, 0.0, 1.0))
        assert np.all(gap <= fwd_bar), (gap.max(), fwd_bar)
    for a, b, what in zip(big, small, WHAT):
        assert torch.equal(a[:pr.BATCH], b), what
    _assert_twins(big, small, index, "tiled")
    index = index[::-1].copy()
    _assert_twins(_run(name, dtype_name, index=index), small, index, "reversed")
    # In those two batches every workgroup holds live rows among the 256 its first pass reads, so the second pass decides
    # nothing.  Here it decides: workgroups 0 and 1 own groups 131 072 and 131 073 (rows 524 288 .. 524 292); their first
    # 64 groups hold interior rows only and those last rows need a second launch.  Were the second pass missing or aimed at
    # another group, the two workgroups would leave and those rows keep no answer.
    seeded_iters = _np(small[1])
    index, first_pass, second_pass = sw.scan_second_pass_index(seeded_iters, B, geometry.grid)
    assert list(second_pass) == list(range(524288, 524293))
    assert np.all(seeded_iters[index[first_pass]] == 0) and np.all(seeded_iters[index[second_pass]] > pr.CHUNK)
    for b in (0, 1):                                             # (all the rows of workgroup b but its 65th group's)
        own = np.concatenate([np.arange(4 * g, min(4 * g + 4, B)) for g in range(b, geometry.groups, geometry.grid)])
        assert own.size in (260, 257) and np.all(seeded_iters[index[own[:256]]] == 0)
        assert np.all(seeded_iters[index[own[256:]]] > pr.CHUNK)
    _assert_twins(_run(name, dtype_name, index=index), small, index, "second pass alone")


# ------------------------------------------------------------------ 4. whole-tile states, tile kernel
@pytest.mark.parametrize("name", ["t7_n8", "k8_n5_ragged_equalities"])
def test_whole_tile_states(name):
    """161 rows: a tile of interior rows (it leaves at the start of the second launch without having iterated), a tile of
    rows that all finish in the earliest launch (k8_n5_ragged_equalities: inside the first; t7_n8, where no row outside
    takes fewer than 33 iterations: the earliest there is) and leaves while its neighbours go on, then the leading 97
    seeded rows: three tiles that need several launches and a ragged one."""
    small = _seeded(name, F32, "tile")
    iters = _np(small[1])
    inside, early, late = sw.launch_classes(iters[:sw.BATCH])
    if name == "k8_n5_ragged_equalities":
        assert iters[early].max() <= pr.CHUNK
    index = np.concatenate((np.resize(inside, 32), np.resize(early, 32), np.arange(sw.BATCH)))
    assert len(index) == sw.BATCH + 64
    big = _run(name, F32, "tile", index=index)
    _assert_twins(big, small, index, "tiles")
    z, it, _, grad = (_np(t)[64:] for t in big)
    assert _compare(name, F32, z, grad, it, rows=sw.BATCH) == []
    # and with the kinds of tile in the opposite order, the ragged tile's rows first in memory
    index = index[::-1].copy()
    _assert_twins(_run(name, F32, "tile", index=index), small, index, "tiles reversed")


# ------------------------------------------------------------------ 5. backward edges
EDGE_RUNS = [(F32, "wave"), (F64, "wave"), (F32, "tile")]


@pytest.mark.parametrize("dtype_name,kernel", EDGE_RUNS)
def test_backward_scaling_is_exact(dtype_name, kernel):
    name = "m65"
    z, iters, vstar, grad = _seeded(name, dtype_name, kernel)
    _, g = _inputs(name, dtype_name)
    _, _, _, max_iters, eps = _family(name)
    pack = _pack(name)
    for power in (40, -40):
        scaled = ops.proj_backward_raw(g * 2.0 ** power, vstar, iters, pack, max_iters, eps[dtype_name], kernel=kernel)
        assert torch.equal(scaled, grad * 2.0 ** power), power
    # a zero gradient and one with a NaN, each on an interior row and on a row outside
    inside, outside = torch.nonzero(iters == 0)[:, 0].tolist(), torch.nonzero(iters > 0)[:, 0].tolist()
    zero_rows, nan_rows = [inside[0], outside[3]], [inside[1], outside[7]]
    edge = g.clone()
    edge[zero_rows] = 0.0
    edge[nan_rows[0], 2] = float("nan")
    edge[nan_rows[1], 0] = float("nan")
    out = ops.proj_backward_raw(edge, vstar, iters, pack, max_iters, eps[dtype_name], kernel=kernel)
    assert torch.all(out[zero_rows] == 0.0)
    assert bool(torch.isnan(out[nan_rows[0], 2])) and bool(torch.isnan(out[nan_rows[1], 0]))
    keep = torch.ones(sw.BATCH, dtype=torch.bool, device="cuda")
    keep[zero_rows + nan_rows] = False
    assert torch.equal(out[keep], grad[keep])                # (a NaN stays in its own row)


@pytest.mark.parametrize("dtype_name,kernel", EDGE_RUNS)
def test_a_nan_row_keeps_to_itself_forward_and_backward(dtype_name, kernel):
    name, row = "m65", 13
    base = _seeded(name, dtype_name, kernel)
    q, g = _inputs(name, dtype_name)
    assert int(base[1][row]) > 0
    q[row, 1] = float("nan")
    out = _run(name, dtype_name, kernel, q=q, g=g)
    # the tile kernel's maxima keep a NaN, so its row runs to the cap; the wave kernel's fmax drops one, and the idle lanes
    # (n < 64) hold dx = 0: its row stops at once.  Either way it answers NaN, reports iterations and touches no other row
    assert torch.all(torch.isnan(out[0][row]))
    assert int(out[1][row]) == (pr.MAX_ITERS if kernel == "tile" else 1)
    keep = torch.arange(sw.BATCH, device="cuda") != row
    for a, b, what in zip(out, base, WHAT):
        assert torch.equal(a[keep], b[keep]), what
    assert not torch.any(torch.isnan(out[3][keep]))


@pytest.mark.parametrize("dtype_name,kernel", EDGE_RUNS)
def test_strided_q_and_g_give_the_contiguous_bits(dtype_name, kernel):
    name = "m65"
    base = _seeded(name, dtype_name, kernel)
    q, g = _inputs(name, dtype_name)
    wide_q = torch.full((sw.BATCH, q.shape[1] + 3), 7.0, device="cuda", dtype=q.dtype)
    wide_g = torch.full((sw.BATCH, g.shape[1] + 5), float("nan"), device="cuda", dtype=g.dtype)
    wide_q[:, :q.shape[1]] = q
    wide_g[:, :g.shape[1]] = g
    qs, gs = wide_q[:, :q.shape[1]], wide_g[:, :g.shape[1]]
    assert qs.stride(0) == q.shape[1] + 3 and gs.stride(0) == g.shape[1] + 5 and not gs.is_contiguous()
    out = _run(name, dtype_name, kernel, q=qs, g=gs)
    for a, b, what in zip(out, base, WHAT):
        assert torch.equal(a, b), what


# ------------------------------------------------------------------ 6. refusals
def test_thirty_three_cones_go_to_the_tile_kernel():
    assert os.environ.get("RAYEN_STRICT_HIP") == "1"
    name = "soc33"
    pack = _pack(name)
    q, g = _inputs(name, F32)
    for dtype in (torch.float32, torch.float64):
        assert not ops.proj_wave_served(pack, dtype)
        with pytest.raises(_lib.RayenError) as err:
            ops.proj_forward_raw(q.to(dtype), pack, 10, 1e-6)
        assert err.value.code == _lib.E_UNSUPPORTED
    cs, rho = pr.make_cs(name), pr.module_for(name).program.rho          # (rho given: its probing on the host is not repeated)
    for kernel in ("auto", "tile"):
        layer = projection.ProjectionModule(cs, create_map=False, max_iters=pr.MAX_ITERS, eps=pr.EPS[F32], rho=rho,
                                            kernel=kernel).cuda()
        leaf = q.clone().requires_grad_(True)
        z, iters = layer.project(leaf)
        (z * g).sum().backward()
        assert sw.compare(name, F32, _np(z), _np(leaf.grad), _np(iters)) == []
    with pytest.raises(_lib.RayenError):
        projection.ProjectionModule(cs, create_map=False, rho=rho).cuda().project(q)          # the default: wave


# one row past the full layouts: 12 blocks a wave at n <= 32, 10 above
PAST = {"n8_1537_rows": (8, 1537), "n33_1281_rows": (33, 1281)}


@pytest.mark.parametrize("label", list(PAST))
def test_one_row_past_the_full_layouts_is_refused_by_both_kernels(label):
    assert os.environ.get("RAYEN_STRICT_HIP") == "1"
    k, m = PAST[label]
    cs = workloads.build_constraints(workloads.random_lin_quad_soc(k, m, 0, 0, seed=51))
    layer = projection.ProjectionModule(cs, create_map=False, rho=1.0)
    prog = layer.program
    assert (prog.n, prog.m, len(prog.soc_rows)) == (k, m, 0)
    pack = ops.ProjPack(prog.arrays(), torch.cuda.current_device())
    assert not ops.proj_tile_served(pack) and not ops.proj_wave_served(pack, torch.float32)
    q = torch.zeros((5, k), device="cuda")
    for kernel in ("wave", "tile"):
        with pytest.raises(_lib.RayenError) as err:
            ops.proj_forward_raw(q, pack, 10, 1e-6, kernel=kernel)
        assert err.value.code == _lib.E_UNSUPPORTED, kernel
        with pytest.raises(_lib.RayenError) as err:
            ops.proj_backward_raw(q, torch.zeros((5, m), device="cuda"), torch.ones(5, dtype=torch.int32, device="cuda"), pack,
                                  10, 1e-6, kernel=kernel)
        assert err.value.code == _lib.E_UNSUPPORTED, kernel
    for kernel in ("wave", "tile", "auto"):
        with pytest.raises(_lib.RayenError):
            projection.ProjectionModule(cs, create_map=False, rho=1.0, kernel=kernel).cuda().project(q)
