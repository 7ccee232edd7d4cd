"""Host checks of the boundary cases of tests/proj_sweep_cases.py: that each case is the shape, the wave instantiation and
the tile instance its table claims, that its fixture is what the reference says and stays within the kink cap, that the host
mirror passes the comparisons the kernels face, and the restated launch rules the GPU tests size their batches with.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import proj_lmi_reference as plr                             # noqa: E402
import proj_reference as pr                                  # noqa: E402
import proj_sweep_cases as sw                                # noqa: E402
import tile_layout_formulas as tl                            # noqa: E402
from test_proj_reference_host import _defective_run          # noqa: E402

ELEM = {sw.F32: 4, sw.F64: 8}


@pytest.mark.parametrize("name", sw.NAMES)
def test_program_is_the_shape_the_table_claims(name):
    case = sw.BY_NAME[name]
    k, m, nq, ns, r_M, _ = case.args
    prog = pr.module_for(name).program
    assert pr.shape_of(name) == case.shape == (prog.n, m + nq * (k + 2) + ns * (r_M + 1), nq + ns)
    assert prog.m_lin == m and list(prog.soc_rows) == [k + 2] * nq + [r_M + 1] * ns
    assert prog.n == k                                       # no equality: NA_E = I


@pytest.mark.parametrize("name", sw.NAMES)
def test_wave_instantiation_and_served(name):
    case = sw.BY_NAME[name]
    n, m, cones = case.shape
    for dtype_name, elem in ELEM.items():
        assert pr.served(n, m, cones, elem) == (case.R is not None), (name, dtype_name)
        assert sw.wave_lds_bytes(n, m, 0, elem) == pr.lds_bytes(n, m, elem)
    if case.R is not None:
        assert sw.R_of(m) == case.R
    else:
        assert cones > pr.MAX_SOC or m > pr.MAX_ROWS


def test_the_boundaries_the_table_names():
    shape = sw.SHAPE
    assert [shape[name][1] for name in ("m64", "m65", "m192", "m193", "m576")] == [64, 65, 192, 193, pr.MAX_ROWS]
    assert [sw.R_of(m) for m in (1, 64, 65, 192, 193, 576)] == [1, 1, 3, 3, 9, 9]
    assert shape["m64"][1] % 4 == 0 and (shape["m64"][1] | 1) == shape["m64"][1] + 1
    assert shape["soc32"][2] == pr.MAX_SOC and shape["soc33"][2] == pr.MAX_SOC + 1
    # the last cone of m64 ends in lane 63; that of m65 straddles 63 -> 64 with t at i = 64; m192 / m193 end at 191 / 192
    # with a 72-row cone: a lane holds two of its rows
    for name, first, last in (("m64", 54, 63), ("m65", 55, 64), ("m192", 120, 191), ("m193", 121, 192)):
        prog = pr.module_for(name).program
        assert (prog.m - prog.soc_rows[-1], prog.m - 1) == (first, last)
    assert pr.module_for("m192").program.soc_rows[-1] == 72 > 64
    assert pr.module_for("nolin_five_cones").program.m_lin == 0
    # m576 in fp64: 64 KiB of LDS, two workgroups a CU
    assert sw.wave_lds_bytes(8, 576, 0, 8) == 64640


@pytest.mark.parametrize("name", sw.NAMES)
def test_tile_layout_and_instance(name):
    case = sw.BY_NAME[name]
    prog = pr.module_for(name).program
    lay = tl.layout(prog.m_lin, list(prog.soc_rows), tl.max_blocks(prog.n))
    assert lay is not None
    nb, instance = case.tile
    assert lay[3] == nb and sw.tile_instance(nb, prog.n) == instance


def test_tile_boundaries_the_table_names():
    Mp = {name: tl.layout(pr.module_for(name).program.m_lin, list(pr.module_for(name).program.soc_rows))[0]
          for name in ("t2_n8_full", "t12_n8_full", "t10_n33_full")}
    assert Mp == {"t2_n8_full": 256, "t12_n8_full": 1536, "t10_n33_full": 1280}          # no free block
    assert [sw.tile_instance(nb, 8) for nb in (1, 2, 3, 6, 7, 12)] == [(2, 1), (2, 1), (6, 1), (6, 1), (12, 1), (12, 1)]
    assert [sw.tile_instance(nb, 33) for nb in (2, 3, 6, 7, 10)] == [(2, 2), (6, 2), (6, 2), (10, 2), (10, 2)]
    # all six instances have a case that reaches the fp64 reference
    have = {case.tile[1] for case in sw.SWEEP}
    for name in ("n33_padding_lanes", "n64_c3_shape"):
        n, m, cones = pr.SHAPE[name]
        prog = pr.module_for(name).program
        have.add(sw.tile_instance(tl.layout(prog.m_lin, list(prog.soc_rows), tl.max_blocks(n))[3], n))
    assert have == {(2, 1), (6, 1), (12, 1), (2, 2), (6, 2), (10, 2)}
    # one row past the full layouts
    assert tl.layout(1536, [], 12) is not None and tl.layout(1537, [], 12) is None
    assert tl.layout(1280, [], 10) is not None and tl.layout(1281, [], 10) is None


@pytest.mark.parametrize("name", sw.NAMES)
def test_fixture_is_what_the_reference_says(name):
    ref, cs = sw.reference(name), pr.make_cs(name)               # (asserts the inputs are make_inputs')
    q, gy = pr.make_inputs(name, sw.BATCH)
    assert np.array_equal(ref.q, q) and np.array_equal(ref.gy, gy)
    assert ref.z.shape == (sw.BATCH, cs.n) and ref.grad_q.shape == (sw.BATCH, cs.n)
    kinks = int(np.count_nonzero(ref.kink))
    if sw.BY_NAME[name].backward:
        assert kinks <= pr.kink_cap(sw.BATCH) == 2, (name, kinks)
    else:                                                        # kept for the forward alone, and this is why
        assert kinks > pr.kink_cap(sw.BATCH) and np.count_nonzero(~ref.interior) >= 48, (name, kinks)
    assert np.any(ref.interior) and np.count_nonzero(~ref.interior) >= 10
    rows = np.random.default_rng(len(name)).choice(np.flatnonzero(~ref.interior), 3, replace=False)
    z = pr.project_rows(cs, ref.q[rows])
    assert np.max(np.abs(z - ref.z[rows])) <= 1e-9
    gz = ref.gy @ cs.NA_E
    for b, zb in zip(rows, z):
        J, margin = pr.jacobian_row(cs, ref.q[b], zb)
        if margin >= pr.KINK_MARGIN:
            assert np.max(np.abs(J @ gz[b] - ref.grad_q[b])) <= 1e-9 * (1.0 + np.max(np.abs(ref.grad_q[b])))


RUNS = [(name, dtype_name) for name in sw.NAMES for dtype_name in sw.dtype_names(name)]


@pytest.mark.parametrize("name,dtype_name", RUNS)
def test_recorded_mirror_passes_the_comparisons(name, dtype_name):
    run = sw.mirror_run(name, dtype_name)
    assert run.iters.max() < pr.MAX_ITERS
    assert sw.compare(name, dtype_name, run.z, run.grad_q, run.iters) == []
    fwd_bar, bwd_bar, _ = sw.bars(name, dtype_name)
    assert fwd_bar <= 2e3 * pr.EPS[dtype_name] and bwd_bar <= 2e4 * pr.EPS[dtype_name], (fwd_bar, bwd_bar)


def test_the_undamaged_copy_passes_on_m65():
    z, grad, iters = _defective_run("m65", sw.F32, None)
    assert sw.compare("m65", sw.F32, z[:sw.BATCH], grad[:sw.BATCH], iters[:sw.BATCH]) == []


@pytest.mark.parametrize("defect", ["moreau_sign", "soc_derivative_is_a_mask", "no_h_in_the_cone_shift"])
def test_comparisons_catch_a_defect_on_m65(defect):
    z, grad, iters = _defective_run("m65", sw.F32, defect)
    assert sw.compare("m65", sw.F32, z[:sw.BATCH], grad[:sw.BATCH], iters[:sw.BATCH]) != [], defect


def test_a_wrong_wrap_index_shows_on_m65():
    """Row 64 of m65 is the last cone's t, the one row in a lane's second register: a kernel that loses it (reads row 63
    again, say) computes the projection onto another set.  The mirror on that program misses the forward bar."""
    import torch
    from rayen_amd import projection
    prog = pr.module_for("m65").program
    G, h = prog.G.copy(), prog.h.copy()
    G[64], h[64] = G[63], h[63]
    wrong = projection.Program(G, h, prog.m_lin, list(prog.soc_rows), prog.n, prog.rho)
    c = projection.Constants(wrong, torch.float32, torch.device("cpu"))
    q, _ = pr.make_inputs("m65", sw.BATCH)
    z, iters, _ = projection.mirror_forward(c, torch.from_numpy(q).float(), pr.MAX_ITERS, pr.EPS[sw.F32])
    fwd_bar, _, _ = sw.bars("m65", sw.F32)
    assert pr.row_gap(z.double().numpy(), sw.reference("m65").z).max() > fwd_bar


@pytest.mark.parametrize("dtype_name", [sw.F32, sw.F64])
def test_the_lmi_case_at_three_rows_a_lane(dtype_name):
    name = sw.LMI_R3
    n, m, cones, r = sw.LMI_R3_SHAPE
    assert plr.shape_of(name) == sw.LMI_R3_SHAPE and m == r * (r + 1) // 2 and sw.R_of(m) == 3
    assert not any(sw.R_of(plr.SHAPE[c.name][1]) == 3 for c in plr.CASES)          # (no other case with a block has R = 3)
    assert plr.case_served(name, dtype_name)
    assert sw.wave_lds_bytes(n, m, r, ELEM[dtype_name]) == plr.lds_bytes(n, m, r, ELEM[dtype_name])
    ref, run = plr.reference(name), plr.mirror_run(name, dtype_name)
    assert ref.z.shape == (33, n) and np.count_nonzero(ref.kink) <= pr.kink_cap(33)
    assert np.any(ref.interior) and np.count_nonzero(~ref.interior) >= 10
    assert run.iters.max() < plr.MAX_ITERS
    assert plr.compare(name, dtype_name, run.z, run.grad_q, run.iters) == []


def test_the_lmi_stride_fixture_is_what_its_reference_says():
    name = sw.LMI_STRIDE
    live = getattr(plr.reference, "inner", plr.reference)(name)
    ref = sw.install_lmi()
    assert plr.reference(name) is ref and ref.z.shape == live.z.shape == (plr.CASE[name].batch, plr.SHAPE[name][0])
    assert np.max(np.abs(ref.z - live.z)) <= 1e-9 and np.array_equal(ref.interior, live.interior)
    assert np.array_equal(ref.kink, live.kink) and np.array_equal(ref.nullity, live.nullity)
    ok = ~live.kink
    assert np.max(plr.row_gap(ref.grad_q, live.grad_q)[ok]) <= 1e-9
    run = plr.mirror_run(name, sw.F64)
    assert run.iters.max() < plr.MAX_ITERS and plr.compare(name, sw.F64, run.z, run.grad_q, run.iters) == []


# ------------------------------------------------------------------ the launch rules the GPU tests size their batches with
def test_wave_grid_restates_the_launch():
    # n64_c3_shape in fp32: 159 KiB, one workgroup a CU, 256 workgroups
    g = sw.wave_grid(*pr.SHAPE["n64_c3_shape"][:2], 0, 4, sw.stride_batch(256))
    assert (g.per_cu, g.grid, g.groups, g.per_workgroup) == (1, 256, 514, 3) and g.lds <= pr.LDS_LIMIT
    assert sw.stride_batch(256) == 2053 and 2053 % pr.WAVES == 1
    assert sw.wave_grid(*pr.SHAPE["n64_c3_shape"][:2], 0, 4, pr.BATCH).per_workgroup == 1       # (what the suite ran so far)
    # m576 in fp64: two workgroups a CU
    g = sw.wave_grid(8, 576, 0, 8, sw.stride_batch(512))
    assert (g.per_cu, g.grid, g.per_workgroup) == (2, 512, 3)
    # r32_k4 in fp64: 143 KiB with the PSD scratch
    n, m, _, r = plr.SHAPE["r32_k4"]
    assert sw.wave_lds_bytes(n, m, r, 8) == plr.lds_bytes(n, m, r, 8)
    g = sw.wave_grid(n, m, r, 8, 1029)
    assert (g.per_cu, g.grid, g.per_workgroup) == (1, 256, 2) and 140 * 1024 < g.lds <= pr.LDS_LIMIT
    # n3_box: eight workgroups a CU; the scan's second pass starts past 64 * grid groups
    n, m, _ = pr.SHAPE["n3_box"]
    at = pr.WAVES * 64 * 2048
    assert sw.wave_grid(n, m, 0, 4, at).scan_passes == 1 and sw.wave_grid(n, m, 0, 4, at + 1).scan_passes == 2
    g = sw.wave_grid(n, m, 0, 4, sw.SCAN_BATCH)
    assert (g.per_cu, g.grid, g.scan_passes) == (8, 2048, 2) and sw.SCAN_BATCH == 524293
    assert sw.wave_grid(n, m, 0, 8, sw.SCAN_BATCH).scan_passes == 2
    # small batches: one group a workgroup
    for B in (1, 4, 5, 97):
        g = sw.wave_grid(8, 65, 0, 4, B)
        assert g.grid == g.groups == -(-B // 4) and g.per_workgroup == 1


def test_tiled_index_covers_every_seeded_row():
    idx = sw.tiled_index(97, 4101)
    assert idx.shape == (4101,) and idx.min() == 0 and idx.max() == 96
    copies, tail = divmod(4101, 97)
    for k in range(copies):
        assert sorted(idx[97 * k:97 * (k + 1)]) == list(range(97))
    assert list(idx[97 * copies:]) == list(range(tail))
    assert np.array_equal(idx, sw.tiled_index(97, 4101))
    assert not np.array_equal(idx[:97], idx[97:194])
