"""The fp64 fused wide backward without a device: rayen_amd/csrc/rayen_wide_fused_bwd64_layout.h against its Python
restatement (tests/wide_fused_bwd64_cases.py), the conditions under which the GPU tests' inputs exercise what they claim to,
the ``wide_backward='fused64'`` keyword, and the binding against the header.

A small host-only C++ program includes the layout header alone, plans every set of the GPU tests and a grid of
``(n, k, identity, widest, samples)``, and prints; the expectations are computed here.  (The exported plan of a pack needs
a pack, and a pack needs a device: tests/test_gpu_wide_fused_bwd64.py holds it against both.)"""
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

import wide_fused_bwd64_cases as C                            # noqa: E402
import wide_fused64_cases as C64                              # noqa: E402
from helpers import kink_mask                                 # noqa: E402
from oracle import rayen_oracle as oracle                     # noqa: E402
from rayen_amd import _build, _lib, ops, workloads            # noqa: E402
from rayen_amd.constraint_module import ConstraintModule      # noqa: E402
from test_gpu_backward import KINK_GAP                        # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan_jobs():
    """(name, n, k, out_identity, rows of the widest QUAD_FAC / SOC segment, samples) of every plan the probe makes."""
    for name in (*C.CASES, "k1025"):
        c = C.consts(name)
        for samples in (0, 16, 32):
            yield f"{name}/{samples}", c.n, c.k, int(c.out_identity), C.widest_t(c.segments), samples
    for n in (1, 64, 65, 200, 616, 617, 624, 625, 1024, 1025):
        for ident, k in ((1, n), (0, n + 30), (0, 1)):
            for widest in (0, 1, 8, 9, 41, 300):
                for samples in (0, 16, 32, 8):
                    yield f"grid n={n} k={k} I={ident} w={widest} S={samples}", n, k, ident, widest, samples
    # a T tile one word of stride inside LDS and one outside at 16 samples beside n = 1024
    room = (C.LDS // 8 - C.scratch(16) - 16 * (1024 + 2)) // 16 - 2         # words of a T row that still fit
    fits = room // 8 * 8
    yield "t_inside", 1024, 1024, 1, fits, 0
    yield "t_inside_odd", 1024, 1024, 1, fits - 7, 0                        # (the same rp)
    yield "t_outside", 1024, 1024, 1, fits + 1, 0
    # equality rows: the g tile is the binding term (k far beyond n), inside and outside
    kmax = (C.LDS // 8 - C.scratch(16)) // 16 - 2
    yield "g_binding", 160, kmax // 8 * 8, 0, 41, 0
    yield "g_outside", 160, kmax // 8 * 8 + 1, 0, 41, 0


def _run_probe(tmp_path, plans):
    body = [f"  plan({j}, {n}, {k}, {ident}, {widest}, {samples});" for j, (_, n, k, ident, widest, samples) in enumerate(plans)]
    src = tmp_path / "wide_fused_bwd64_probe.cpp"
    src.write_text("""
#include <cstdio>
#include "rayen_wide_fused_bwd64_layout.h"
static void plan(int job, int n, int k, int ident, int widest, int samples) {
  const rayen::WideFusedBwd64Plan p = rayen::wide_fused_bwd64_plan(n, k, ident, widest, samples);
  std::printf("plan %d %d %d %d %d %d %d %d %d %d %lld %d\\n", job, p.kp, p.ks, p.ke, p.gs, p.rp, p.ts, p.np, p.samples,
              p.region_words, (long long)p.lds_bytes, p.served);
}
int main() {
  std::printf("consts %d %lld %d %d\\n", rayen::kWideFusedBwd64MaxN, (long long)rayen::kWideFusedBwd64Lds,
              rayen::wide_fused_bwd64_scratch(16), rayen::wide_fused_bwd64_scratch(32));
  std::printf("ws %lld %lld %lld\\n", (long long)rayen::wide_fused_bwd_workspace(1, 300),
              (long long)rayen::wide_fused_bwd_workspace(2, 300), (long long)rayen::wide_fused_bwd_perm_offset(65));
""" + "\n".join(body) + "\n  return 0;\n}\n")
    exe = tmp_path / "wide_fused_bwd64_probe"
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    built = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", _build.CSRC, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stderr)
    return [line.split() for line in ran.stdout.strip().splitlines()]


def test_layout_matches_the_restatement(tmp_path):
    plans = list(_plan_jobs())
    out = _run_probe(tmp_path, plans)
    assert out[0] == ["consts", str(C.MAX_N), str(C.LDS), str(C.scratch(16)), str(C.scratch(32))]
    # the grouping's workspace is the fp32 backward's, as it is
    assert [int(x) for x in out[1][1:]] == [C.workspace(1, 300), C.workspace(2, 300), C.perm_offset(65)] == [0, 256 + 1200, 512]
    got = {int(f[1]): dict(zip(C.PLAN_KEYS, (int(x) for x in f[2:]))) for f in out if f[0] == "plan"}
    assert len(got) == len(plans)
    served, tile = {}, {}
    for j, (name, n, k, ident, widest, samples) in enumerate(plans):
        want = C.plan(n, k, ident, widest, samples)
        assert got[j] == want, name
        p = got[j]
        S = p["samples"]
        served[name], tile[name] = p["served"], S
        assert S in (16, 32) and (samples not in (16, 32) or S == samples), name
        # K padded to 8, strides whose half is odd, the tiles as documented, in 8-byte words
        assert p["kp"] % 8 == 0 and 0 <= p["kp"] - n < 8 and p["ks"] == p["kp"] + 2 and (p["ks"] // 2) % 2 == 1, name
        assert (p["ke"], p["gs"]) == ((0, 0) if ident else ((k + 7) // 8 * 8, (k + 7) // 8 * 8 + 2)), name
        assert (p["rp"], p["ts"]) == ((0, 0) if widest == 0 else ((widest + 7) // 8 * 8, (widest + 7) // 8 * 8 + 2)), name
        assert ident or (p["gs"] // 2) % 2 == 1, name
        assert widest == 0 or (p["ts"] // 2) % 2 == 1, name
        assert p["np"] % 16 == 0 and 0 <= p["np"] - n < 16, name
        assert p["lds_bytes"] == 8 * (max(S * p["gs"], S * (p["ks"] + p["ts"])) + 10 * S), name
        assert p["served"] == int(1 <= n <= 1024 and samples in (0, 16, 32) and p["lds_bytes"] <= C.LDS), name
        assert p["region_words"] == (max(S * p["gs"], S * (p["ks"] + p["ts"])) if p["served"] else 0), name
        # S as the forward chooses it: 32 where that plan fits, else 16 (free choice)
        if samples == 0 and 1 <= n <= 1024:
            assert S == (32 if C.plan(n, k, ident, widest, 32)["served"] else 16), name
    assert all(served[f"{name}/0"] and served[f"{name}/16"] for name in C.CASES)
    assert served["k1025/0"] == served["k1025/16"] == served["k1025/32"] == 0
    assert served["t_inside"] == 1 and served["t_inside_odd"] == 1 and served["t_outside"] == 0
    assert tile["t_inside"] == tile["g_binding"] == 16
    inside, outside = (got[[p[0] for p in plans].index(x)] for x in ("t_inside", "t_outside"))
    assert inside["lds_bytes"] <= C.LDS < outside["lds_bytes"] == inside["lds_bytes"] + 8 * 16 * 8
    assert served["g_binding"] == 1 and served["g_outside"] == 0
    g = got[[p[0] for p in plans].index("g_binding")]
    assert 16 * g["gs"] > 16 * (g["ks"] + g["ts"]) and g["region_words"] == 16 * g["gs"]
    # the edge of the 32-sample tile, and a forced 32 beyond it
    assert tile["s32_last/0"] == 32 and tile["s16_first/0"] == 16 and C.consts("s16_first").n == C.consts("s32_last").n + 1
    assert served["s32_last/32"] == 1 and served["s16_first/32"] == 0 and served["k1024/32"] == 0 and tile["k1024/0"] == 16
    assert all(tile[f"{name}/0"] == 32 for name in (*C.MIXED, *C.SMALL))


def test_the_cases_are_what_their_names_promise():
    # the edge family's segment table does not depend on n: the search of s32_last_n() holds on the sets built
    a, b, probe = C.consts("s32_last"), C.consts("s16_first"), C64.packed("s32_last")
    table = lambda c: [(s.type, s.row0, s.nrows, s.aux_row) for s in c.segments]          # noqa: E731
    assert table(a) == table(b) == table(probe) and C.widest_t(a.segments) == 5 and a.out_identity and b.out_identity
    assert a.n == C.s32_last_n() and C.plan_of(a)["samples"] == 32 and C.plan_of(b)["samples"] == 16
    # (the backward's edge is not the forward's: the T tile and the scratch differ)
    assert C.s32_last_n() != C64.s32_last_n()
    c = C.consts("n65")
    assert c.n == ops._WIDE_MIN_N[torch.float64] == 65 and C.plan_of(c)["kp"] // 8 % 4 == 1
    assert sorted(s.nrows % 16 for s in c.segments) == [1, 1, 1]
    c = C.consts("plan_a")
    assert any(s.type == _lib.SEG_SOC and s.aux_row == 15 for s in c.segments)
    assert [s.nrows for s in C.consts("plan_c").segments if s.type == _lib.SEG_QUAD_FAC] == list(C64.FAC_ROWS)
    c = C.consts("mixE")
    assert c.n == 160 and c.k == 190 and not c.out_identity and c.k % 16 == 14
    assert sorted(s.nrows for s in c.segments if s.type == _lib.SEG_QUAD_FAC) == [4, 38] and C.consts("mixI").out_identity
    c = C.consts("k1024")
    assert c.n == 1024 and any(s.type == _lib.SEG_QUAD_SYM and s.nrows == 1024 for s in c.segments)
    assert C.consts("k1025").n == 1025
    for name in C.CASES:
        assert C.inputs(name).shape == (300, C.consts(name).n) and C.inputs(name).dtype == torch.float64, name
        assert C.grads(name).shape == (300, C.consts(name).k) and C.grads(name).dtype == torch.float64, name


@pytest.mark.parametrize("name", C.CASES)
def test_the_inputs_exercise_what_the_gpu_tests_rely_on(name):
    """Conditions, not measurements: which constraint is active where, in fp64 from the packed constants, and the kink rows
    of the reference alone (``helpers.kink_mask`` at ``KINK_GAP[float64]``).

    Every non-linear SEGMENT is active on at least 3 non-kink rows in the cases whose inputs are this file's to choose (n65,
    plan_a, plan_c, the two edges).  mixI, mixE and k1024 keep the inputs of tests/wide_fused_bwd_cases.py: there every segment
    TYPE the set has is active on at least 3 non-kink rows, bar the cone of k1024, which no input of that family activates
    (the dense quadratic dominates it; the case is the dense QUAD_SYM at the envelope's last n).  The segments these inputs
    leave out run on hand-set ``active`` records instead:
    tests/test_gpu_wide_fused_bwd64.py::test_segments_no_input_activates_run_on_hand_set_records."""
    c, cov = C.consts(name), C.coverage(name)
    kink = kink_mask(oracle, C.cs(name), C.inputs(name).unsqueeze(2), KINK_GAP[torch.float64])
    good = {i: int((~kink[rows]).sum()) for i, rows in cov["rows"].items()}
    print(f"{name}: clipped {cov['clipped']} of 300, non-kink active rows by segment "
          f"{[(c.segments[i].type, c.segments[i].nrows, g) for i, g in good.items()]}, distinct non-linear active segments "
          f"per tile of 16 {cov['per_tile']}, unclipped tiles {cov['unclipped_tiles']}, kink rows {int(kink.sum())}")
    assert kink.sum() <= 0.02 * kink.size, name               # (the cap inside _assert_gradient: it holds for the reference alone)
    by_type = {}
    for i, g in good.items():
        by_type[c.segments[i].type] = by_type.get(c.segments[i].type, 0) + g
    if name in (*C.SMALL, *C.EDGES):
        assert all(g >= 3 for i, g in good.items() if c.segments[i].type != _lib.SEG_LIN), (name, good)
    elif name in C.MIXED:
        assert all(by_type.get(t, 0) >= 3 for t in (_lib.SEG_LIN, _lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC, _lib.SEG_SOC)), by_type
    else:
        assert by_type[_lib.SEG_QUAD_SYM] >= 3 and by_type[_lib.SEG_LIN] >= 3, by_type
    assert 0 < cov["clipped"] < 300
    if name != "k1024":
        assert cov["unclipped_tiles"] >= 1 and cov["per_tile"][6] == cov["per_tile"][7] == 0, name      # rows 96-127
    if name in (*C.MIXED, *C.SMALL):
        assert max(cov["per_tile"]) >= 2, name                # a tile of 16 walks at least two segments


def _small():
    return workloads.build_constraints(workloads.random_lin_quad_soc(k=5, m=7, n_quad=1, n_soc=1, seed=3))


def test_constructor_and_backward_raw_refuse_unknown_and_misplaced_values():
    cs = _small()
    assert ops.WIDE_BACKWARDS == ("products", "fused", "fused64") and "auto" not in ops.WIDE_BACKWARDS
    assert ConstraintModule(cs, create_map=False).wide_backward == "products"
    assert ConstraintModule(cs, create_map=False, wide_backward="fused64").wide_backward == "fused64"
    for bad in ("auto", "fused32", "Fused64", None, 64):
        with pytest.raises(ValueError):
            ConstraintModule(cs, create_map=False, wide_backward=bad)
    for method in ("RAYEN_old", "UU", "Bar"):
        with pytest.raises(ValueError):
            ConstraintModule(workloads.build_constraints(workloads.random_lin_quad_soc(k=3, m=7, n_quad=0, n_soc=0, seed=3)),
                             create_map=False, method=method, wide_backward="fused64")
    with pytest.raises(ValueError):
        ops.backward_raw(torch.zeros(1, 5, dtype=torch.float64), None, None, torch.zeros(1, 5, dtype=torch.float64), None,
                         wide_backward="fused32")
    # the route key: every pair with the fp64 fused backward has one of its own; the others keep theirs
    assert ConstraintModule(cs, create_map=False)._route_key() is False
    assert ConstraintModule(cs, create_map=False, wide_backward="fused64")._route_key() == "products+bwd_fused64"
    assert ConstraintModule(cs, create_map=False, wide_kernel="fused64", wide_backward="fused64")._route_key() == "fused64+bwd_fused64"
    assert ConstraintModule(cs, create_map=False, wide_backward="fused")._route_key() == "products+bwd_fused"


def test_pickles_and_host_tensors():
    cs = _small()
    layer = ConstraintModule(cs, create_map=False, wide_kernel="fused64", wide_backward="fused64")
    again = pickle.loads(pickle.dumps(layer))
    assert again.wide_backward == "fused64" and again.wide_kernel == "fused64" and again._route_key() == "fused64+bwd_fused64"
    state = layer.__getstate__()
    del state["wide_backward"], state["wide_kernel"]                   # a pickle from before the keywords
    old = ConstraintModule.__new__(ConstraintModule)
    old.__setstate__(state)
    assert old.wide_backward == "products" and old.wide_kernel == "products" and old._route_key() is False
    # host tensors (and n = 5, far from the wide route): the keyword does nothing
    x = torch.linspace(-1, 1, 10, dtype=torch.float64).reshape(2, 5, 1)
    grads = []
    for m in (again, ConstraintModule(cs, create_map=False)):
        xg = x.clone().requires_grad_(True)
        y = m(xg)
        y.sum().backward()
        grads.append((y.detach(), xg.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def test_binding_and_header_declare_the_same_entry_points(tmp_path):
    text = open(os.path.join(REPO, "include", "rayen_hip_wide_fused_bwd64.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.EXPORTS_WIDE_FUSED_BWD64) and len(declared) == 4
    others = (_lib.EXPORTS, _lib.EXPORTS_TILE, _lib.EXPORTS_TILE64, _lib.EXPORTS_DC3_TILE, _lib.EXPORTS_DC3_TILE64,
              _lib.EXPORTS_COST_STREAM, _lib.EXPORTS_BAR_STREAM, _lib.EXPORTS_WIDE_FUSED, _lib.EXPORTS_WIDE_FUSED_BWD,
              _lib.EXPORTS_WIDE_FUSED64)
    assert all(not set(declared) & set(o) for o in others)
    main_header = open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    assert '#include "rayen_hip_wide_fused_bwd64.h"' in main_header
    assert re.search(r"#define RAYEN_ABI_VERSION 15\b", main_header) and _lib.ABI_VERSION == 15
    assert "rayen_wide_fused_bwd64.hip" in _build.SOURCES and "-fno-slp-vectorize" in _build.EXTRA_FLAGS["rayen_wide_fused_bwd64.hip"]
    lib = _lib.load()
    assert lib.rayen_abi_version() == 15
    for name in declared:
        assert hasattr(lib, name), name
    # argument checks that need no device
    out = (ctypes.c_int64 * 11)()
    assert lib.rayen_wide_fused_bwd64_served(None) == 0
    assert lib.rayen_wide_fused_bwd64_plan(None, 0, out) == -1
    assert lib.rayen_wide_fused_bwd64_workspace_bytes(None, 300) == 0
    assert lib.rayen_ray_project_wide_fused_bwd_f64(None, None, 0, 1, None, None, None, 1, None, 1, None, 0, 0, None) == -1
    assert lib.rayen_wide_fused_bwd_served(None, 1) == 0            # 'fused' stays fp32 only
    assert hasattr(torch.ops.rayen_amd, "ray_project_wide") and hasattr(torch.ops.rayen_amd, "ray_project_bwd_wide_fused64")
    # the public header in a C99 translation unit
    src = tmp_path / "c99.c"
    src.write_text('#include "rayen_hip.h"\nint main(void) { return rayen_wide_fused_bwd64_served(0) != 0; }\n')
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the image"
    built = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(REPO, "include"),
                            str(src)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
