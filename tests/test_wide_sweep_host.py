"""The wide kernels' sweep without a device: ``wide_sweep_cases.relayout`` moves rows and nothing else (fp64, 1e-12), every
crafted case has the plan and the coverage its name promises (conditions, restated from ``wide_fused_cases.plan`` /
``wide_fused_bwd_cases.plan`` and the fp64 ``active64``), and the launchers' grids as the two ``*_cases`` modules restate
them against a small host-only C++ program over rayen_launch_geometry.h and the two layout headers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_fused_bwd_cases as WB                             # noqa: E402
import wide_fused_cases as F                                  # noqa: E402
import wide_sweep_cases as S                                  # noqa: E402
from rayen_amd import _build, _lib                            # noqa: E402

LIN, SYM, FAC, SOC = _lib.SEG_LIN, _lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC, _lib.SEG_SOC
NONLINEAR = (SYM, FAC, SOC)


def _v(name):
    return S.inputs(name)[:, :, 0].double().numpy()


def _blocks(s):
    return range(s.row0 // 32, (s.row0 + s.nrows - 1) // 32 + 1)


def _aux_rows(s):
    return range(s.aux_row, s.aux_row + S.naux(s.type))


def _clipped_on(name):
    """Clipped rows by active segment, fp64."""
    return S.coverage(name)["by_seg"]


@pytest.mark.parametrize("name", S.CASES)
def test_relayout_moves_rows_and_nothing_else(name):
    p, c = S.packed(name), S.consts(name)
    v = _v(name)
    y0, k0, a0 = S.evaluate64(p, v)
    y1, k1, a1 = S.evaluate64(c, v)
    assert np.max(np.abs(k1 - k0) / np.maximum(1.0, k0)) <= 1e-12
    assert np.max(np.abs(y1 - y0) / np.maximum(1.0, np.abs(y0))) <= 1e-12
    origin = np.array(c.origin + [-1])
    assert np.array_equal(origin[a1], a0)
    # the rows themselves: every segment's rows and aux rows are those of the segment it came from, bit for bit (a linear
    # segment: a piece of the run, copies apart), no two placements overlap, and what is left is poisoned
    used = np.zeros(c.W.shape[0], dtype=int)
    for s, o in zip(c.segments, c.origin):
        so = p.segments[o]
        assert (s.type, s.f0, s.f1) == (so.type, so.f0, so.f1)
        rows, rows_o = c.W[s.row0:s.row0 + s.nrows], p.W[so.row0:so.row0 + so.nrows]
        if s.type == LIN:
            have = {r.tobytes() for r in rows_o}
            assert all(r.tobytes() in have for r in rows)
        else:
            assert np.array_equal(rows, rows_o)
            assert np.array_equal(c.W[s.aux_row:s.aux_row + S.naux(s.type)], p.W[so.aux_row:so.aux_row + S.naux(s.type)])
            used[list(_aux_rows(s))] += 1
        used[s.row0:s.row0 + s.nrows] += 1
    lin_rows = {r.tobytes() for s in c.segments if s.type == LIN for r in c.W[s.row0:s.row0 + s.nrows]}
    lin_rows_o = {r.tobytes() for s in p.segments if s.type == LIN for r in p.W[s.row0:s.row0 + s.nrows]}
    assert lin_rows == lin_rows_o
    assert used.max() == 1 and sorted(np.flatnonzero(used == 0).tolist()) == sorted(c.gap_rows)
    assert np.all(c.W[c.gap_rows] == S.POISON)
    # the fp64 gradient follows (row 8: v = 0)
    g0 = S.truth_grad(p, v, S.grads(name).double().numpy())
    g1 = S.truth(name)[3]
    assert np.all(np.isfinite(g1))
    assert np.max(np.abs(g1 - g0)) <= 1e-12 * max(1.0, np.max(np.abs(g0)))


@pytest.mark.parametrize("name", S.CASES)
def test_inputs_cover_both_sides_and_few_kinks(name):
    cov = S.coverage(name)
    c = S.consts(name)
    fp, sp, bp = S.plans(c)
    print(f"{name}: n {c.n} k {c.k} rows {c.W.shape[0]} nb_w {fp['nb_w']} clipped {cov['clipped']} of {S.B}, by type "
          f"{cov['by_type']}, by segment {cov['by_seg']}, non-linear keys per tile {cov['nl_keys_per_tile']}, kink rows {cov['kinks']}")
    assert c.n > 128 and fp["served"] == 1 and bp["served"] == 1
    assert 4 * cov["clipped"] >= S.B and 4 * (S.B - cov["clipped"]) >= S.B
    assert cov["kinks"] <= 3
    kappa = S.truth(name)[1]
    assert kappa[8] == 0 and np.all(kappa[:4] < 1) and np.all(kappa[4:8] > 1)
    assert np.any(kappa > 1.05) and np.any((kappa > 0) & (kappa < 0.95))          # (kappa on both sides of 1)
    for s in c.segments:
        if s.type == SOC:
            assert s.f1 < 0


@pytest.mark.parametrize("name", list(S.NBW))
def test_nbw_plans(name):
    c = S.consts(name)
    fp, sp, _ = S.plans(c)
    assert c.n == 129 and c.out_identity and fp["nb_w"] == int(name[3:])
    lin = [s for s in c.segments if s.type == LIN]
    assert len(lin) == 1
    s = lin[0]
    owning = [w for w in range(4) if F.block_start(fp["nb_w"], w) < F.block_start(fp["nb_w"], w + 1)]
    assert len(owning) == min(4, fp["nb_w"])
    owners = {F.wave_of(fp["nb_w"], b) for b in _blocks(s)}
    assert owners <= set(owning) and len(owners) >= min(3, len(owning))
    assert s.row0 % 32 != 0 and (s.row0 + s.nrows) % 32 != 0
    sizes = sorted(F.block_start(fp["nb_w"], w + 1) - F.block_start(fp["nb_w"], w) for w in range(4))
    assert sizes == {2: [0, 0, 1, 1], 3: [0, 1, 1, 1], 5: [1, 1, 1, 2], 7: [1, 2, 2, 2]}[fp["nb_w"]]


def test_fac_edges_plan():
    c = S.consts("fac_edges")
    assert c.n == 135
    fac = [(i, s) for i, s in enumerate(c.segments) if s.type == FAC]
    assert sorted(s.nrows for _, s in fac) == [1, 31, 32, 33]
    assert any(s.row0 % 32 == 31 for _, s in fac)
    on = _clipped_on("fac_edges")
    assert all(on[i] >= 3 for i, _ in fac), on


def test_aux_far_plan():
    c = S.consts("aux_far")
    fp, _, _ = S.plans(c)
    assert c.n == 136
    nl = [s for s in c.segments if s.type in NONLINEAR]
    assert sorted(s.type for s in nl) == sorted(NONLINEAR)
    for s in nl:
        owners = {F.wave_of(fp["nb_w"], b) for b in _blocks(s)}
        for r in _aux_rows(s):
            assert r > s.row0 + s.nrows - 1
            assert r // 32 not in _blocks(s) and F.wave_of(fp["nb_w"], r // 32) not in owners


def test_soc_straddle_plan():
    c = S.consts("soc_straddle")
    fp, _, bp = S.plans(c)
    assert c.n == 161 and bp["np"] // 32 == 6
    hit = [i for i, s in enumerate(c.segments) if s.type == SOC and s.aux_row % 32 == 31
           and F.wave_of(fp["nb_w"], s.aux_row // 32) != F.wave_of(fp["nb_w"], (s.aux_row + 1) // 32)]
    assert hit
    on = _clipped_on("soc_straddle")
    assert any(on[i] >= 3 for i in hit), on


def test_gaps_plan():
    c = S.consts("gaps")
    fp, _, bp = S.plans(c)
    assert c.n == 200 and bp["np"] // 32 == 7
    gap = set(c.gap_rows)
    # a block that one segment's rows fill has no room for a row of nobody: every OTHER block holds one (a QUAD_SYM has n
    # consecutive rows: five whole blocks here)
    for b in range(fp["nb_w"]):
        rows = set(range(32 * b, min(32 * b + 32, c.W.shape[0])))
        filled = any(rows <= set(range(s.row0, s.row0 + s.nrows)) for s in c.segments)
        assert filled or (rows & gap), b
        assert filled or (rows - gap), b                  # (and rows of a segment beside it)
    lin = [s for s in c.segments if s.type == LIN]
    assert len(lin) == 2
    for s in lin:
        assert s.row0 - 1 in gap and s.row0 + s.nrows in gap
    sym = [s for s in c.segments if s.type == SYM]
    assert sym
    for s in sym:
        between = set(range(s.aux_row + 1, s.row0))
        assert between and between <= gap
    assert {s.type for s in c.segments} == {LIN, SYM, FAC, SOC}
    # the same pack with the rows of nobody zero: nothing else differs
    z = S.zero_gaps(c)
    keep = np.ones(c.W.shape[0], dtype=bool)
    keep[c.gap_rows] = False
    assert np.array_equal(z.W[keep], c.W[keep]) and not z.W[~keep].any() and z.segments == c.segments


def _pairs(c):
    """(lower row, higher row) of W of every pair of identical linear rows."""
    seen, out = {}, []
    for s in c.segments:
        if s.type != LIN:
            continue
        for r in range(s.row0, s.row0 + s.nrows):
            key = c.W[r].tobytes()
            if key in seen:
                out.append((seen[key], r))
            else:
                seen[key] = r
    return sorted(out)


@pytest.mark.parametrize("name", ["lin_ties", "lin_ties_cut"])
def test_lin_ties_plan(name):
    c = S.consts(name)
    fp, _, _ = S.plans(c)
    assert c.n == 129
    pairs = _pairs(c)
    assert len(pairs) == 3
    wave = lambda r: F.wave_of(fp["nb_w"], r // 32)          # noqa: E731
    same_block = [(a, b) for a, b in pairs if a // 32 == b // 32]
    same_wave = [(a, b) for a, b in pairs if a // 32 < b // 32 and wave(a) == wave(b)]
    later_wave = [(a, b) for a, b in pairs if wave(a) < wave(b)]
    assert len(same_block) == 1 and len(same_wave) == 1 and len(later_wave) == 1
    assert ((same_block[0][0] >> 2) & 1) != ((same_block[0][1] >> 2) & 1)          # the other half-wave
    # every copied row is the fp64 maximiser on at least five inputs (found on the LOWER row: argmax keeps the first)
    v = _v(name)
    T = v @ c.W.T
    lin_rows = np.concatenate([np.arange(s.row0, s.row0 + s.nrows) for s in c.segments if s.type == LIN])
    kappa = S.truth(name)[1]
    best_row = lin_rows[np.argmax(T[:, lin_rows], axis=1)]
    lin_active = (kappa > 0) & (np.max(T[:, lin_rows], axis=1) == kappa)
    for a, b in pairs:
        assert int(np.sum(lin_active & (best_row == a))) >= 5, (a, b)
    lin = [s for s in c.segments if s.type == LIN]
    if name == "lin_ties":
        assert len(lin) == 1
    else:
        assert len(lin) == 2 and lin[0].row0 + lin[0].nrows == lin[1].row0
        a, b = later_wave[0]
        assert a < lin[1].row0 <= b                     # the pair across the cut: the earlier SEGMENT wins the tie
    # without the copies: the packer's layout
    assert len(_pairs(S.consts("lin_ties_plain"))) == 0


def test_eq_k_plans():
    n_nl, ragged = {}, 0
    for name, k in S.EQ_K.items():
        c = S.consts(name)
        fp, _, bp = S.plans(c)
        assert (c.n, c.k, bool(c.out_identity)) == (160, k, False)
        assert bp["ke"] == (k + 7) // 8 * 8 and fp["nb_e"] == 6
        ragged += int(k % 32 != 0)
        n_nl[name] = sum(s.type != LIN for s in c.segments)
    assert [k % 32 for k in S.EQ_K.values()] == [1, 31, 0] and sorted(k % 8 for k in S.EQ_K.values()) == [0, 1, 7]
    assert ragged == 2
    assert n_nl["eq_k161"] == 0 and n_nl["eq_k191"] == 1 and n_nl["eq_k192"] >= 2
    assert WB.workspace(n_nl["eq_k161"], S.B) == 0 and WB.workspace(n_nl["eq_k191"], S.B) == 0
    assert WB.workspace(n_nl["eq_k192"], S.B) > 0
    assert _clipped_on("eq_k191")[1] >= 3


def test_nl5_plan():
    c = S.consts("nl5")
    assert c.n == 136
    nl = [i for i, s in enumerate(c.segments) if s.type in NONLINEAR]
    assert len(nl) == 5
    on = _clipped_on("nl5")
    assert all(on[i] >= 1 for i in nl), on
    assert max(S.coverage("nl5")["nl_keys_per_tile"]) >= 4


def test_output_blocks_of_the_backward_cover_every_residue():
    """``nbo = np / 32`` output blocks dealt ``ob = wave; ob += 4``: the cases cover the residues 1, 2, 3 of nbo modulo 4 (0
    is k1024 of tests/wide_fused_bwd_cases.py, nbo = 32), and n % 8 in {0, 7} sits next to n % 32 != 0."""
    nbo = {name: S.plans(S.consts(name))[2]["np"] // 32 for name in S.CASES}
    assert {v % 4 for v in nbo.values()} == {1, 2, 3}, nbo
    assert WB.plan(1024, 1024, 1, 0)["np"] // 32 == 32
    ns = {S.consts(name).n for name in S.CASES}
    assert any(n % 8 == 7 and n % 32 for n in ns) and any(n % 8 == 0 and n % 32 for n in ns)


# ---------------------------------------------------------------- the launchers' grids
CUS = (256, 128, 248, 1, 304)
BATCHES = (1, 97, 300, 32 * 640 + 13, 262144 + 333)


def _grid_jobs():
    names = [(S.consts(name), name) for name in S.CASES]
    import wide_fused_bwd_cases as WBC
    from rayen_amd.constraint_module import ConstraintModule
    for name in WBC.CASES:
        names.append((ConstraintModule(WBC.cs(name), create_map=False).packed_constants(), name))
    for c, name in names:
        yield name, c


def test_slots_and_grids_match_the_headers(tmp_path):
    jobs = list(_grid_jobs())
    body = []
    for j, (name, c) in enumerate(jobs):
        segs = ", ".join(f"{{{a}, {b}, {cc}, {d}}}" for a, b, cc, d in F.seg_inputs(c.segments))
        body.append(f"  {{ static const rayen::WideFusedSegIn segs[] = {{{segs}}};\n"
                    f"    job({j}, {c.n}, {c.k}, {c.W.shape[0]}, {int(c.out_identity)}, segs, {len(c.segments)}, "
                    f"{WB.widest_t(c.segments)}); }}")
    src = tmp_path / "wide_grid_probe.cpp"
    src.write_text("""
#include <cstdio>
#include "rayen_launch_geometry.h"
#include "rayen_wide_fused_layout.h"
#include "rayen_wide_fused_bwd_layout.h"
static const int cus[] = {""" + ", ".join(map(str, CUS)) + """};
static const long long batches[] = {""" + ", ".join(f"{b}ll" for b in BATCHES) + """};
// the launchers' own lines (rayen_wide_fused.hip, rayen_wide_fused_bwd.hip): workgroups a CU holds by LDS, capped by what
// the registers allow, times the CUs the grid may fill
static long long slots_of(long long lds_bytes, int cap, int n_cus) {
  long long per_cu = (160 * 1024) / lds_bytes;
  per_cu = per_cu < 1 ? 1 : (per_cu > cap ? cap : per_cu);
  return (long long)n_cus * per_cu;
}
static void job(int j, int n, int k, int n_rows, int ident, const rayen::WideFusedSegIn* segs, int n_seg, int widest) {
  const rayen::WideFusedPlan f = rayen::wide_fused_plan(n, k, n_rows, ident, segs, n_seg, nullptr);
  const rayen::WideFusedBwdPlan b = rayen::wide_fused_bwd_plan(n, k, ident, widest);
  for (int c : cus) {
    const long long sf = slots_of(f.lds_bytes, 4, c), sb = slots_of(b.lds_bytes, 3, c);
    std::printf("%d %d %lld %lld", j, c, sf, sb);
    for (long long B : batches)
      std::printf(" %lld %lld", (long long)rayen::persistent_grid(B, rayen::kWideFusedTile, sf, 1),
                  (long long)rayen::persistent_grid(B, 32, sb, 1));
    std::printf("\\n");
  }
}
int main() {
""" + "\n".join(body) + "\n  return 0;\n}\n")
    exe = tmp_path / "wide_grid_probe"
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    built = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", _build.CSRC, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stderr)
    lines = [[int(x) for x in line.split()] for line in ran.stdout.strip().splitlines()]
    assert len(lines) == len(jobs) * len(CUS)
    per_cu_seen = set()
    for got in lines:
        name, c = jobs[got[0]]
        cus = got[1]
        fp, _, bp = S.plans(c)
        sf, sb = F.slots_fwd(fp, cus), WB.slots_bwd(bp, cus)
        want = [got[0], cus, sf, sb]
        for B in BATCHES:
            want += [F.grid(B, sf), F.grid(B, sb)]
        assert got == want, (name, cus)
        per_cu_seen.add((sf // cus, sb // cus))
    assert {p[0] for p in per_cu_seen} >= {1, 4} and {p[1] for p in per_cu_seen} >= {1, 3}
    # the reserved compute units enter through launch_simds(): all but the reserved ones, at least one
    assert [F.launch_cus(256, r) for r in (0, 8, 128)] == [256, 248, 128] and F.launch_cus(64, 128) == 1
    assert WB.grouping_grid(300, 128) == 2 and WB.grouping_grid(2 * 256 * 512 + 256 + 77, 128) == 512


def test_second_round_batches_take_second_rounds():
    """The batch sizes of the GPU file's second rounds, from the restated grids, on the part the suite runs on and on a
    smaller one: more than two rounds and a partial last tile."""
    for cus in (256, 304, 64):
        half = F.launch_cus(cus, 128)
        for name in ("mixI", "mixE", "k1024"):
            from rayen_amd.constraint_module import ConstraintModule
            c = ConstraintModule(WB.cs(name), create_map=False).packed_constants()
            fp, _, bp = S.plans(c)
            for slots in (F.slots_fwd(fp, half), WB.slots_bwd(bp, half)):
                B = S.second_round_batch(slots)
                n_tiles = -(-B // 32)
                assert n_tiles > 2 * F.grid(B, slots) and B % 32 == 13
