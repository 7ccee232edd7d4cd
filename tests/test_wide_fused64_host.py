"""The fp64 fused wide forward without a device: the block plan of rayen_amd/csrc/rayen_wide_fused64_layout.h against its
Python restatement (tests/wide_fused64_cases.py) and against the properties it promises, the crafted plans of the GPU tests,
the module's ``wide_kernel='fused64'`` and the binding against the header.

A small host-only C++ program includes the header alone, plans every set of the GPU tests (free choice of the tile, and
both forced sizes) and a few shapes around the limits, and prints the plans; the expectations are computed here."""
import ctypes
import os
import pickle
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_fused64_cases as C                                # noqa: E402
import wide_sweep_cases as WS                                 # noqa: E402
from rayen_amd import _build, _lib, ops, workloads            # noqa: E402
from rayen_amd.constraint_module import ConstraintModule      # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _jobs():
    """(name, n, k, n_rows, out_identity, segments, samples) of every plan the probe makes."""
    for name in (*C.CASES, "k1025", "plan_e_plain"):
        c = C.consts(name)
        for samples in (0, 16, 32):
            yield f"{name}/{samples}", c.n, c.k, c.W.shape[0], int(c.out_identity), C.seg_inputs(c.segments), samples
    for rows in (1, 15, 16, 17, 63, 64, 65):
        yield f"lin{rows}", 200, 200, rows, 1, [(0, rows, 2, 0)], 0
        # the same rows as a cone's, behind two aux rows and one linear row: every reduction crosses the same boundaries
        yield f"soc{rows}", 200, 230, rows + 3, 0, [(0, 1, 2, 0), (3, rows, 1, 2)], 0
    yield "n1024", 1024, 1024, 64, 1, [(0, 64, 2, 0)], 0
    yield "n1025", 1025, 1025, 64, 1, [(0, 64, 2, 0)], 0
    # n inside, the scratch beyond LDS even at 16 samples: 600 cones of one row, each in a block of its own
    yield "scratch", 1024, 1024, 9600, 1, [(16 * i, 1, 1, 2) for i in range(600)], 0
    yield "samples8", 200, 200, 64, 1, [(0, 64, 2, 0)], 8


def _run_probe(tmp_path, jobs):
    blocks = []
    for j, (_, n, k, n_rows, ident, segs, samples) in enumerate(jobs):
        rows = ", ".join(f"{{{a}, {b}, {c}, {d}}}" for a, b, c, d in segs)
        blocks.append(f"  {{ static const rayen::WideFusedSegIn segs[] = {{{rows}}};\n"
                      f"    plan({j}, {n}, {k}, {n_rows}, {ident}, segs, {len(segs)}, {samples}); }}")
    src = tmp_path / "wide_fused64_probe.cpp"
    src.write_text("""
#include <cstdio>
#include <vector>
#include "rayen_wide_fused64_layout.h"
static void plan(int job, int n, int k, int n_rows, int ident, const rayen::WideFusedSegIn* segs, int n_seg, int samples) {
  std::vector<rayen::WideFusedSegPlan> sp((size_t)n_seg);
  const rayen::WideFused64Plan p = rayen::wide_fused64_plan(n, k, n_rows, ident, segs, n_seg, sp.data(), samples);
  std::printf("job %d %d %d %d %d %d %d %d %d %d %d %lld %lld %d\\n", job, p.n, p.kp, p.ks, p.samples, p.rows_w_pad, p.nb_w,
              p.rows_e_pad, p.nb_e, p.rows_pad, p.scratch_words, (long long)p.tile_bytes, (long long)p.lds_bytes, p.served);
  for (const auto& s : sp)
    std::printf("s %d %d %d %d %d %d\\n", s.first_block, s.last_block, s.wave_first, s.wave_last, s.part_off, s.aux_off);
}
int main() {
  std::printf("consts %d %d %d %lld\\n", rayen::kWideFused64Block, rayen::kWideFusedWaves, rayen::kWideFused64MaxN,
              (long long)rayen::kWideFused64Lds);
""" + "\n".join(blocks) + "\n  return 0;\n}\n")
    exe = tmp_path / "wide_fused64_probe"
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    built = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", _build.CSRC, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stderr)
    lines = ran.stdout.strip().splitlines()
    assert lines[0].split() == ["consts", str(C.BLOCK), str(C.WAVES), str(C.MAX_N), str(C.LDS)]
    got, cur = {}, None
    for line in lines[1:]:
        f = line.split()
        if f[0] == "job":
            cur = got[int(f[1])] = dict(plan=dict(zip(C.PLAN_KEYS, (int(x) for x in f[2:]))), segs=[])
        else:
            keys = ("first_block", "last_block", "wave_first", "wave_last", "part_off", "aux_off")
            cur["segs"].append(dict(zip(keys, (int(x) for x in f[1:]))))
    return got


def test_plan_matches_the_restatement_and_keeps_its_promises(tmp_path):
    jobs = list(_jobs())
    got = _run_probe(tmp_path, jobs)
    assert len(got) == len(jobs)
    idle_wave = crossing = False
    for j, (name, n, k, n_rows, ident, segs, samples) in enumerate(jobs):
        want, want_segs = C.plan(n, k, n_rows, ident, segs, samples)
        g = got[j]
        assert g["plan"] == want, name
        assert g["segs"] == want_segs, name
        p = g["plan"]
        S = p["samples"]
        assert S in (16, 32) and (samples not in (16, 32) or S == samples), name
        # rows padded to 16, the two parts apart; K padded to 8 with a stride whose half is odd
        assert p["rows_w_pad"] % 16 == 0 and 0 <= p["rows_w_pad"] - n_rows < 16, name
        assert p["rows_e_pad"] == (0 if ident else (k + 15) // 16 * 16) and p["rows_pad"] == p["rows_w_pad"] + p["rows_e_pad"], name
        assert p["kp"] % 8 == 0 and 0 <= p["kp"] - n < 8 and p["ks"] == p["kp"] + 2 and (p["ks"] // 2) % 2 == 1, name
        # every block -- so every row -- belongs to exactly one wave, in contiguous rising runs
        for nb in (p["nb_w"], p["nb_e"]):
            owners = [[w for w in range(C.WAVES) if C.block_start(nb, w) <= b < C.block_start(nb, w + 1)] for b in range(nb)]
            assert all(len(o) == 1 for o in owners), name
            flat = [o[0] for o in owners]
            assert flat == sorted(flat), name
            sizes = [flat.count(w) for w in range(C.WAVES)]
            assert max(sizes) - min(sizes) <= 1, name
            idle_wave |= 0 < nb < C.WAVES
        # segment block ranges; scratch regions disjoint, inside the scratch and filling it
        regions = []
        for (row0, nrows, slots, naux), s in zip(segs, g["segs"]):
            if nrows:
                assert s["first_block"] * 16 <= row0 < s["first_block"] * 16 + 16, name
                assert s["last_block"] * 16 <= row0 + nrows - 1 < s["last_block"] * 16 + 16, name
                assert s["wave_first"] == C.wave_of(p["nb_w"], s["first_block"]), name
                assert s["wave_last"] == C.wave_of(p["nb_w"], s["last_block"]), name
                crossing |= s["wave_last"] > s["wave_first"]
            else:
                assert s["last_block"] < s["first_block"] and s["wave_last"] < s["wave_first"], name
            regions.append((s["part_off"], s["part_off"] + (s["wave_last"] - s["wave_first"] + 1) * slots * S))
            regions.append((s["aux_off"], s["aux_off"] + naux * S))
        regions = [r for r in regions if r[1] > r[0]]
        assert all(a[1] <= b[0] for a, b in zip(sorted(regions), sorted(regions)[1:])), name
        assert all(0 <= lo and hi <= p["scratch_words"] for lo, hi in regions), name
        assert sum(hi - lo for lo, hi in regions) == p["scratch_words"], name
        # LDS as documented: the tile, the scratch, two values a sample -- all in doubles
        assert p["tile_bytes"] == 8 * S * p["ks"] and p["lds_bytes"] == p["tile_bytes"] + 8 * p["scratch_words"] + 16 * S, name
        assert p["served"] == int(1 <= n <= 1024 and samples in (0, 16, 32) and p["lds_bytes"] <= C.LDS), name
        # S as documented: 32 where that plan fits, else 16 (free choice)
        if samples == 0 and 1 <= n <= 1024:
            fits32 = C.plan(n, k, n_rows, ident, segs, 32)[0]["served"]
            assert S == (32 if fits32 else 16), name
    assert idle_wave and crossing
    served = {name: got[j]["plan"]["served"] for j, (name, *_) in enumerate(jobs)}
    tile = {name: got[j]["plan"]["samples"] for j, (name, *_) in enumerate(jobs)}
    assert all(served[f"{name}/0"] and served[f"{name}/16"] for name in C.CASES)
    assert served["n1024"] == 1 and served["n1025"] == 0 and served["scratch"] == 0 and served["samples8"] == 0
    assert served["k1025/0"] == 0 and served["k1025/16"] == 0
    # the edge of the 32-sample tile, and a forced 32 beyond it
    assert tile["s32_last/0"] == 32 and tile["s16_first/0"] == 16 and C.consts("s16_first").n == C.consts("s32_last").n + 1
    assert served["s32_last/32"] == 1 and served["s16_first/32"] == 0 and served["k1024/32"] == 0 and tile["k1024/0"] == 16


def test_the_crafted_plans_are_what_their_names_promise():
    seg_of = lambda c, t: [s for s in c.segments if s.type == t]           # noqa: E731
    # n65: one past the threshold, a K tail of one group, every segment one row past a block
    c = C.consts("n65")
    assert c.n == ops._WIDE_MIN_N[torch.float64] == 65 and C.plan_of(c)[0]["kp"] // 8 % 4 == 1
    assert sorted(s.nrows % 16 for s in c.segments) == [1, 1, 1] and len({s.type for s in c.segments}) == 3
    c = C.consts("n66_one_row")
    assert c.W.shape[0] == 1 and C.plan_of(c)[0]["nb_w"] == 1
    c = C.consts("k190_n160")
    assert not c.out_identity and c.k % 16 == 14 and c.n == 160
    assert C.consts("k1024").n == 1024 and C.consts("k1025").n == 1025
    # plan A: a cone's aux rows at 15 | 16, two blocks, two waves
    c = C.consts("plan_a")
    nb = C.plan_of(c)[0]["nb_w"]
    assert any(s.aux_row == 15 for s in seg_of(c, _lib.SEG_SOC)) and C.wave_of(nb, 0) != C.wave_of(nb, 1)
    # plan B: 2, 3, 5, 7 blocks
    assert [C.plan_of(C.consts(name))[0]["nb_w"] for name in C.PLAN_B] == [2, 3, 5, 7]
    # plan C: a one-row QUAD_FAC among its four
    assert [s.nrows for s in seg_of(C.consts("plan_c"), _lib.SEG_QUAD_FAC)] == list(C.FAC_ROWS) and 1 in C.FAC_ROWS
    # plan D: a row of nobody, POISON, in every block that one segment does not fill
    c = C.consts("plan_d")
    gap = set(c.gap_rows)
    assert gap and all(np.all(c.W[r] == WS.POISON) for r in gap)
    owner = {}
    for i, s in enumerate(c.segments):
        for r in list(range(s.row0, s.row0 + s.nrows)) + list(range(s.aux_row, s.aux_row + WS.naux(s.type))):
            owner[r] = (i, r >= s.row0)
    assert set(owner) | gap == set(range(c.W.shape[0]))
    for b in range(C.plan_of(c)[0]["nb_w"]):
        rows = range(16 * b, min(16 * b + 16, c.W.shape[0]))
        filled = len(rows) == 16 and len({owner.get(r) for r in rows}) == 1 and owner.get(rows[0], (0, False))[1]
        assert filled or any(r in gap for r in rows), b
    # plan E: exact copies inside a block, across blocks, and across the cut
    for name, pairs in (("plan_e", ((40, 45), (104, 142), (7, 76))), ("plan_e_cut", ((40, 45), (104, 142), (7, 76)))):
        c = C.consts(name)
        for lo, hi in pairs:
            assert np.array_equal(c.W[lo], c.W[hi]), (name, lo, hi)
    assert 40 // 16 == 45 // 16 and 104 // 16 != 142 // 16
    cut = C.consts("plan_e_cut").segments
    assert cut[0].type == cut[1].type == _lib.SEG_LIN and cut[0].nrows == WS.TIE_CUT and 7 < WS.TIE_CUT <= 76


def test_constructor_accepts_fused64_and_still_refuses_auto():
    cs = workloads.build_constraints(workloads.random_lin_quad_soc(k=5, m=7, n_quad=1, n_soc=1, seed=3))
    assert "fused64" in ops.WIDE_KERNELS and "auto" not in ops.WIDE_KERNELS
    assert ConstraintModule(cs, create_map=False).wide_kernel == "products"
    layer = ConstraintModule(cs, create_map=False, wide_kernel="fused64")
    assert layer.wide_kernel == "fused64" and layer.wide_backward == "products" and layer._route_key() == "fused64"
    for bad in ("auto", "fused32", None, 64):
        with pytest.raises(ValueError):
            ConstraintModule(cs, create_map=False, wide_kernel=bad)
    for method in ("RAYEN_old", "UU", "Bar"):
        with pytest.raises(ValueError):
            ConstraintModule(workloads.build_constraints(workloads.random_lin_quad_soc(k=3, m=7, n_quad=0, n_soc=0, seed=3)),
                             create_map=False, method=method, wide_kernel="fused64")
    with pytest.raises(ValueError):
        ops.project_raw(torch.zeros(1, 5, dtype=torch.float64), None, wide_kernel="auto")
    assert ConstraintModule(cs, create_map=False, wide_kernel="fused64", wide_backward="fused")._route_key() == "fused64+bwd_fused"


def test_pickle_round_trip_and_old_pickles():
    cs = workloads.build_constraints(workloads.random_lin_quad_soc(k=5, m=7, n_quad=1, n_soc=1, seed=3))
    layer = ConstraintModule(cs, create_map=False, wide_kernel="fused64")
    again = pickle.loads(pickle.dumps(layer))
    assert again.wide_kernel == "fused64" and again._route_key() == "fused64"
    x = torch.linspace(-1, 1, 10).reshape(2, 5, 1)
    assert torch.equal(again(x), ConstraintModule(cs, create_map=False)(x))          # host tensors: the same evaluator
    state = layer.__getstate__()
    del state["wide_kernel"]                           # a pickle from before the keyword
    old = ConstraintModule.__new__(ConstraintModule)
    old.__setstate__(state)
    assert old.wide_kernel == "products" and old._route_key() is False


def test_binding_and_header_declare_the_same_entry_points():
    text = open(os.path.join(REPO, "include", "rayen_hip_wide_fused64.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.EXPORTS_WIDE_FUSED64)
    others = (_lib.EXPORTS, _lib.EXPORTS_TILE, _lib.EXPORTS_TILE64, _lib.EXPORTS_DC3_TILE, _lib.EXPORTS_DC3_TILE64,
              _lib.EXPORTS_COST_STREAM, _lib.EXPORTS_BAR_STREAM, _lib.EXPORTS_WIDE_FUSED, _lib.EXPORTS_WIDE_FUSED_BWD)
    assert all(not set(declared) & set(o) for o in others)
    main_header = open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    assert '#include "rayen_hip_wide_fused64.h"' in main_header
    assert re.search(r"RAYEN_KERNEL_WIDE_FUSED64\s*=\s*%d\b" % _lib.KERNEL_WIDE_FUSED64, main_header) and _lib.KERNEL_WIDE_FUSED64 == 13
    assert re.search(r"#define RAYEN_ABI_VERSION 15\b", main_header) and _lib.ABI_VERSION == 15
    assert "rayen_wide_fused64.hip" in _build.SOURCES and "-fno-slp-vectorize" in _build.EXTRA_FLAGS["rayen_wide_fused64.hip"]
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    # argument checks that need no device
    out = (ctypes.c_int64 * 13)()
    assert lib.rayen_wide_fused64_served(None) == 0
    assert lib.rayen_wide_fused64_plan(None, 0, out) == -1
    assert lib.rayen_ray_project_wide_fused64_f64(None, None, 0, 1, None, 1, None, None, None, 0, None) == -1
    assert lib.rayen_wide_fused_served(None, 1) == 0            # 'fused' stays fp32 only
