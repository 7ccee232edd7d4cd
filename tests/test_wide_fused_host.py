"""The fused wide forward without a device: the block plan of rayen_amd/csrc/rayen_wide_fused_layout.h against its Python
restatement (tests/wide_fused_cases.py) and against the properties it promises, the module's ``wide_kernel`` keyword, and
the binding against the header.

A small host-only C++ program includes the header alone, plans every set of the GPU tests and a few row counts around the
block size, and prints the plans; the expectations are computed here."""
import os
import pickle
import re
import shutil
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_fused_cases as C                                  # noqa: E402
from rayen_amd import _build, _lib, ops, workloads            # noqa: E402
from rayen_amd.constraint_module import ConstraintModule      # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _jobs():
    """(name, n, k, n_rows, out_identity, segments) of every plan the probe makes."""
    for name in C.CASES:
        consts = ConstraintModule(C.cs(name), create_map=False).packed_constants()
        yield name, consts.n, consts.k, consts.W.shape[0], int(consts.out_identity), C.seg_inputs(consts.segments)
    for rows in (1, 31, 32, 33, 127, 128, 129):
        yield f"lin{rows}", 200, 200, rows, 1, [(0, rows, 2, 0)]
        # the same rows as a cone's, behind two aux rows and one linear row: every reduction crosses the same boundaries
        yield f"soc{rows}", 200, 230, rows + 3, 0, [(0, 1, 2, 0), (3, rows, 1, 2)]
    yield "n1024", 1024, 1024, 64, 1, [(0, 64, 2, 0)]
    yield "n1025", 1025, 1025, 64, 1, [(0, 64, 2, 0)]
    # n inside, the scratch beyond LDS: 300 cones of one row, each in a block of its own
    yield "scratch", 1024, 1024, 9600, 1, [(32 * i, 1, 1, 2) for i in range(300)]


def _run_probe(tmp_path, jobs):
    blocks = []
    for j, (_, n, k, n_rows, ident, segs) in enumerate(jobs):
        rows = ", ".join(f"{{{a}, {b}, {c}, {d}}}" for a, b, c, d in segs)
        blocks.append(f"  {{ static const rayen::WideFusedSegIn segs[] = {{{rows}}};\n"
                      f"    plan({j}, {n}, {k}, {n_rows}, {ident}, segs, {len(segs)}); }}")
    src = tmp_path / "wide_fused_probe.cpp"
    src.write_text("""
#include <cstdio>
#include <vector>
#include "rayen_wide_fused_layout.h"
static void plan(int job, int n, int k, int n_rows, int ident, const rayen::WideFusedSegIn* segs, int n_seg) {
  std::vector<rayen::WideFusedSegPlan> sp((size_t)n_seg);
  const rayen::WideFusedPlan p = rayen::wide_fused_plan(n, k, n_rows, ident, segs, n_seg, sp.data());
  std::printf("job %d %d %d %d %d %d %d %d %d %d %lld %lld %d\\n", job, p.n, p.kp, p.ks, p.rows_w_pad, p.nb_w, p.rows_e_pad,
              p.nb_e, p.rows_pad, p.scratch_words, (long long)p.tile_bytes, (long long)p.lds_bytes, p.served);
  for (const auto& s : sp)
    std::printf("s %d %d %d %d %d %d\\n", s.first_block, s.last_block, s.wave_first, s.wave_last, s.part_off, s.aux_off);
  std::printf("w");
  for (int b = 0; b < p.nb_w; ++b) std::printf(" %d", rayen::wide_fused_wave_of(p.nb_w, b));
  std::printf("\\n");
}
int main() {
  std::printf("consts %d %d %d %lld\\n", rayen::kWideFusedTile, rayen::kWideFusedWaves, rayen::kWideFusedMaxN,
              (long long)rayen::kWideFusedLds);
""" + "\n".join(blocks) + "\n  return 0;\n}\n")
    exe = tmp_path / "wide_fused_probe"
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    built = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", _build.CSRC, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stderr)
    lines = ran.stdout.strip().splitlines()
    assert lines[0].split() == ["consts", str(C.TILE), str(C.WAVES), str(C.MAX_N), str(C.LDS)]
    got, cur = {}, None
    for line in lines[1:]:
        f = line.split()
        if f[0] == "job":
            keys = ("n", "kp", "ks", "rows_w_pad", "nb_w", "rows_e_pad", "nb_e", "rows_pad", "scratch_words", "tile_bytes",
                    "lds_bytes", "served")
            cur = got[int(f[1])] = dict(plan=dict(zip(keys, (int(x) for x in f[2:]))), segs=[], waves=None)
        elif f[0] == "s":
            keys = ("first_block", "last_block", "wave_first", "wave_last", "part_off", "aux_off")
            cur["segs"].append(dict(zip(keys, (int(x) for x in f[1:]))))
        else:
            cur["waves"] = [int(x) for x in f[1:]]
    return got


def test_plan_matches_the_restatement_and_keeps_its_promises(tmp_path):
    jobs = list(_jobs())
    got = _run_probe(tmp_path, jobs)
    assert len(got) == len(jobs)
    idle_wave = crossing = False
    for j, (name, n, k, n_rows, ident, segs) in enumerate(jobs):
        want, want_segs = C.plan(n, k, n_rows, ident, segs)
        g = got[j]
        assert g["plan"] == want, name
        assert g["segs"] == want_segs, name
        p = g["plan"]
        # rows padded to 32, the two parts apart; K padded to 8 with a stride whose quarter is odd
        assert p["rows_w_pad"] % 32 == 0 and 0 <= p["rows_w_pad"] - n_rows < 32, name
        assert p["rows_e_pad"] == (0 if ident else (k + 31) // 32 * 32) and p["rows_pad"] == p["rows_w_pad"] + p["rows_e_pad"], name
        assert p["kp"] % 8 == 0 and 0 <= p["kp"] - n < 8 and p["ks"] == p["kp"] + 4 and (p["ks"] // 4) % 2 == 1, name
        # every block -- so every row -- belongs to exactly one wave, in contiguous rising runs
        for nb in (p["nb_w"], p["nb_e"]):
            owners = [[w for w in range(C.WAVES) if C.block_start(nb, w) <= b < C.block_start(nb, w + 1)] for b in range(nb)]
            assert all(len(o) == 1 for o in owners), name
            flat = [o[0] for o in owners]
            assert flat == sorted(flat), name
            sizes = [flat.count(w) for w in range(C.WAVES)]
            assert max(sizes) - min(sizes) <= 1, name
            idle_wave |= 0 < nb < C.WAVES
        assert g["waves"] == [C.wave_of(p["nb_w"], b) for b in range(p["nb_w"])], name
        # segment block ranges; scratch regions disjoint and inside the scratch
        regions = []
        for (row0, nrows, slots, naux), s in zip(segs, g["segs"]):
            if nrows:
                assert s["first_block"] * 32 <= row0 < s["first_block"] * 32 + 32, name
                assert s["last_block"] * 32 <= row0 + nrows - 1 < s["last_block"] * 32 + 32, name
                assert s["wave_first"] == g["waves"][s["first_block"]] and s["wave_last"] == g["waves"][s["last_block"]], name
                crossing |= s["wave_last"] > s["wave_first"]
            else:
                assert s["last_block"] < s["first_block"] and s["wave_last"] < s["wave_first"], name
            regions.append((s["part_off"], s["part_off"] + (s["wave_last"] - s["wave_first"] + 1) * slots * 32))
            regions.append((s["aux_off"], s["aux_off"] + naux * 32))
        regions = [r for r in regions if r[1] > r[0]]
        assert all(a[1] <= b[0] for a, b in zip(sorted(regions), sorted(regions)[1:])), name
        assert all(0 <= lo and hi <= p["scratch_words"] for lo, hi in regions), name
        assert sum(hi - lo for lo, hi in regions) == p["scratch_words"], name
        # LDS as documented: the tile, the scratch, two values a sample
        assert p["tile_bytes"] == 4 * 32 * p["ks"] and p["lds_bytes"] == p["tile_bytes"] + 4 * p["scratch_words"] + 256, name
        assert p["served"] == int(n <= 1024 and p["lds_bytes"] <= C.LDS), name
    assert idle_wave and crossing
    served = {name: got[j]["plan"]["served"] for j, (name, *_) in enumerate(jobs)}
    assert all(served[name] for name in C.CASES)
    assert served["n1024"] == 1 and served["n1025"] == 0 and served["scratch"] == 0


def test_constructor_refuses_unknown_and_misplaced_values():
    cs = workloads.build_constraints(workloads.random_lin_quad_soc(k=5, m=7, n_quad=1, n_soc=1, seed=3))
    assert ConstraintModule(cs, create_map=False).wide_kernel == "products"
    assert ConstraintModule(cs, create_map=False, wide_kernel="fused").wide_kernel == "fused"
    for bad in ("auto", "bogus", None, 1):
        with pytest.raises(ValueError):
            ConstraintModule(cs, create_map=False, wide_kernel=bad)
    for method in ("RAYEN_old", "UU", "Bar"):
        with pytest.raises(ValueError):
            ConstraintModule(workloads.build_constraints(workloads.random_lin_quad_soc(k=3, m=7, n_quad=0, n_soc=0, seed=3)),
                             create_map=False, method=method, wide_kernel="fused")
    with pytest.raises(ValueError):
        ops.project_raw(torch.zeros(1, 5), None, wide_kernel="auto")
    # the route key: the default keeps the keys it had, the fused route has one of its own
    assert ConstraintModule(cs, create_map=False)._route_key() is False
    assert ConstraintModule(cs, create_map=False, wide_kernel="fused")._route_key() == "fused"


def test_pickle_round_trip_and_old_pickles():
    cs = workloads.build_constraints(workloads.random_lin_quad_soc(k=5, m=7, n_quad=1, n_soc=1, seed=3))
    layer = ConstraintModule(cs, create_map=False, wide_kernel="fused")
    again = pickle.loads(pickle.dumps(layer))
    assert again.wide_kernel == "fused" and again._route_key() == "fused"
    x = torch.linspace(-1, 1, 10).reshape(2, 5, 1)
    assert torch.equal(again(x), ConstraintModule(cs, create_map=False)(x))          # host tensors: the same evaluator
    state = layer.__getstate__()
    del state["wide_kernel"]                           # a pickle from before the keyword
    old = ConstraintModule.__new__(ConstraintModule)
    old.__setstate__(state)
    assert old.wide_kernel == "products" and old._route_key() is False


def test_binding_and_header_declare_the_same_entry_points():
    text = open(os.path.join(REPO, "include", "rayen_hip_wide_fused.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.EXPORTS_WIDE_FUSED)
    assert not set(declared) & set(_lib.EXPORTS)
    main_header = open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    assert '#include "rayen_hip_wide_fused.h"' in main_header
    assert re.search(r"RAYEN_KERNEL_WIDE_FUSED\s*=\s*%d\b" % _lib.KERNEL_WIDE_FUSED, main_header)
    assert re.search(r"#define RAYEN_ABI_VERSION 15\b", main_header) and _lib.ABI_VERSION == 15
    assert "rayen_wide_fused.hip" in _build.SOURCES and "-fno-slp-vectorize" in _build.EXTRA_FLAGS["rayen_wide_fused.hip"]
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    # argument checks that need no device
    assert lib.rayen_wide_fused_served(None, 0) == 0 and lib.rayen_wide_fused_served(None, 1) == 0
    assert lib.rayen_ray_project_wide_fused_f32(None, None, 0, 1, None, 1, None, None, None, None) == -1
    assert hasattr(torch.ops.rayen_amd, "ray_project_wide_fused")
