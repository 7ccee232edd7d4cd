"""The fused wide backward without a device: rayen_amd/csrc/rayen_wide_fused_bwd_layout.h against its Python restatement
(tests/wide_fused_bwd_cases.py), the conditions under which the GPU tests' inputs exercise what they claim to, the
``wide_backward`` keyword, and the binding against the header.

A small host-only C++ program includes the layout header alone, plans every set of the GPU tests and a few probe sizes,
scans random bucket counts, and prints; the expectations are computed here."""
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

import wide_fused_bwd_cases as C                              # noqa: E402
from helpers import kink_mask                                 # noqa: E402
from oracle import rayen_oracle as oracle                     # noqa: E402
from rayen_amd import _build, _lib, ops, workloads            # noqa: E402
from rayen_amd.constraint_module import ConstraintModule      # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _consts(name):
    return ConstraintModule(C.cs(name), create_map=False).packed_constants()


def _plan_jobs():
    """(name, n, k, out_identity, rows of the widest QUAD_FAC / SOC segment) of every plan the probe makes."""
    for name in C.CASES:
        consts = _consts(name)
        yield name, consts.n, consts.k, int(consts.out_identity), C.widest_t(consts.segments)
    yield "n1024", 1024, 1024, 1, 0
    yield "n1025", 1025, 1025, 1, 0
    yield "n1", 1, 1, 1, 0
    # a T tile one word of stride inside LDS and one outside: the largest rp (a multiple of 8) that fits beside n = 1024
    room = (C.LDS // 4 - C.SCRATCH - 32 * (1024 + 4)) // 32 - 4           # words of a T row that still fit
    fits = room // 8 * 8
    yield "t_inside", 1024, 1024, 1, fits
    yield "t_inside_odd", 1024, 1024, 1, fits - 7                         # (the same rp)
    yield "t_outside", 1024, 1024, 1, fits + 1
    # equality rows: the g tile is the binding term (k far beyond n), inside and outside
    kmax = (C.LDS // 4 - C.SCRATCH) // 32 - 4
    yield "g_binding", 160, kmax // 8 * 8, 0, 41
    yield "g_outside", 160, kmax // 8 * 8 + 1, 0, 41


def _scan_jobs():
    rng = np.random.default_rng(5)
    jobs = [("random", rng.integers(0, 50, 37).tolist()), ("empty buckets", [5, 0, 0, 7, 0, 1, 0, 0]),
            ("one bucket holds everything", [0, 0, 300, 0]), ("one key", [300]),
            ("more keys than threads", rng.integers(0, 3, 1000).tolist())]
    return jobs


def _run_probe(tmp_path, plans, scans):
    body = [f"  plan({j}, {n}, {k}, {ident}, {widest});" for j, (_, n, k, ident, widest) in enumerate(plans)]
    for j, (_, counts) in enumerate(scans):
        body.append(f"  {{ int32_t c[] = {{{', '.join(str(c) for c in counts)}}}; scan({j}, c, {len(counts)}); }}")
    src = tmp_path / "wide_fused_bwd_probe.cpp"
    src.write_text("""
#include <cstdio>
#include "rayen_wide_fused_bwd_layout.h"
static void plan(int job, int n, int k, int ident, int widest) {
  const rayen::WideFusedBwdPlan p = rayen::wide_fused_bwd_plan(n, k, ident, widest);
  std::printf("plan %d %d %d %d %d %d %d %d %d %lld %d\\n", job, p.kp, p.ks, p.ke, p.gs, p.rp, p.ts, p.np, p.region_words,
              (long long)p.lds_bytes, p.served);
}
static void scan(int job, int32_t* counts, int n_keys) {
  rayen::wide_fused_bwd_scan(counts, n_keys, 256);
  std::printf("scan %d", job);
  for (int i = 0; i < n_keys; ++i) std::printf(" %d", counts[i]);
  std::printf("\\n");
}
int main() {
  std::printf("consts %d %lld %d\\n", rayen::kWideFusedBwdMaxN, (long long)rayen::kWideFusedBwdLds, rayen::kWideFusedBwdScratch);
  std::printf("ws %lld %lld %lld %lld %lld %lld\\n", (long long)rayen::wide_fused_bwd_workspace(0, 300),
              (long long)rayen::wide_fused_bwd_workspace(1, 300), (long long)rayen::wide_fused_bwd_workspace(2, 300),
              (long long)rayen::wide_fused_bwd_workspace(7, 0), (long long)rayen::wide_fused_bwd_workspace(100, 262144),
              (long long)rayen::wide_fused_bwd_perm_offset(65));
""" + "\n".join(body) + "\n  return 0;\n}\n")
    exe = tmp_path / "wide_fused_bwd_probe"
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    built = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", _build.CSRC, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stderr)
    return [line.split() for line in ran.stdout.strip().splitlines()]


def test_layout_matches_the_restatement(tmp_path):
    plans, scans = list(_plan_jobs()), _scan_jobs()
    out = _run_probe(tmp_path, plans, scans)
    assert out[0] == ["consts", str(C.MAX_N), str(C.LDS), str(C.SCRATCH)]
    assert [int(x) for x in out[1][1:]] == [C.workspace(0, 300), C.workspace(1, 300), C.workspace(2, 300), C.workspace(7, 0),
                                            C.workspace(100, 262144), C.perm_offset(65)]
    assert C.workspace(0, 300) == C.workspace(1, 300) == C.workspace(7, 0) == 0 and C.workspace(2, 300) == 256 + 1200
    keys = ("kp", "ks", "ke", "gs", "rp", "ts", "np", "region_words", "lds_bytes", "served")
    got = {int(f[1]): dict(zip(keys, (int(x) for x in f[2:]))) for f in out if f[0] == "plan"}
    served = {}
    for j, (name, n, k, ident, widest) in enumerate(plans):
        want = C.plan(n, k, ident, widest)
        assert got[j] == want, name
        p = got[j]
        served[name] = p["served"]
        # K padded to 8, strides whose quarter is odd, the tiles as documented
        assert p["kp"] % 8 == 0 and 0 <= p["kp"] - n < 8 and p["ks"] == p["kp"] + 4 and (p["ks"] // 4) % 2 == 1, name
        assert (p["ke"], p["gs"]) == ((0, 0) if ident else ((k + 7) // 8 * 8, (k + 7) // 8 * 8 + 4)), name
        assert (p["rp"], p["ts"]) == ((0, 0) if widest == 0 else ((widest + 7) // 8 * 8, (widest + 7) // 8 * 8 + 4)), name
        assert p["np"] % 32 == 0 and 0 <= p["np"] - n < 32, name
        assert p["lds_bytes"] == 4 * (max(32 * p["gs"], 32 * (p["ks"] + p["ts"])) + C.SCRATCH), name
        assert p["served"] == int(n <= 1024 and p["lds_bytes"] <= C.LDS), name
    assert all(served[name] for name in C.CASES)
    assert served["n1024"] == 1 and served["n1025"] == 0 and served["n1"] == 1
    assert served["t_inside"] == 1 and served["t_inside_odd"] == 1 and served["t_outside"] == 0
    inside, outside = (got[[p[0] for p in plans].index(x)] for x in ("t_inside", "t_outside"))
    assert inside["lds_bytes"] <= C.LDS < outside["lds_bytes"] == inside["lds_bytes"] + 4 * 32 * 8
    assert served["g_binding"] == 1 and served["g_outside"] == 0
    g = got[[p[0] for p in plans].index("g_binding")]
    assert 32 * g["gs"] > 32 * (g["ks"] + g["ts"]) and g["region_words"] == 32 * g["gs"]
    # the scan: counts -> first positions of the buckets
    scanned = {int(f[1]): [int(x) for x in f[2:]] for f in out if f[0] == "scan"}
    for j, (name, counts) in enumerate(scans):
        assert scanned[j] == (np.cumsum([0] + counts)[:-1]).tolist(), name


def test_the_inputs_exercise_what_the_gpu_tests_rely_on():
    """Conditions, not measurements: which constraint is active where, in fp64 from the packed constants."""
    total, wide = {}, {}
    for name in C.CASES:
        cov = C.coverage(name)
        kinks = int(kink_mask(oracle, C.cs(name), C.inputs(name), 1e-4).sum())
        print(f"{name}: clipped {cov['clipped']} of 300, active by type {cov['by_type']}, of those on segments of more than 32 rows "
              f"{cov['wide']}, distinct active segments per tile {cov['per_tile']}, kink rows {kinks}")
        for t, c in cov["by_type"].items():
            total[t] = total.get(t, 0) + c
        for t, c in cov["wide"].items():
            wide[t] = wide.get(t, 0) + c
        assert kinks <= max(2, 0.02 * 300), name
    for t in (_lib.SEG_LIN, _lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC, _lib.SEG_SOC):
        assert total.get(t, 0) >= 8, t
    assert wide.get(_lib.SEG_QUAD_FAC, 0) >= 2 and wide.get(_lib.SEG_SOC, 0) >= 2
    for name in ("mixI", "mixE"):
        cov = C.coverage(name)
        assert max(cov["per_tile"]) >= 4 and cov["unclipped_tiles"] >= 1, name
        assert cov["per_tile"][3] == 0                                  # rows 96-127
    mixE = C.coverage("mixE")
    assert mixE["by_type"].get(_lib.SEG_QUAD_FAC, 0) >= 2 and mixE["by_type"].get(_lib.SEG_SOC, 0) >= 2
    consts = _consts("mixE")
    assert consts.n == 160 and consts.k == 190 and not consts.out_identity
    assert _consts("mixI").out_identity and C.cs("mixI").n == 160


def _small():
    return workloads.build_constraints(workloads.random_lin_quad_soc(k=5, m=7, n_quad=1, n_soc=1, seed=3))


def test_constructor_refuses_unknown_and_misplaced_values():
    cs = _small()
    assert ConstraintModule(cs, create_map=False).wide_backward == "products"
    assert ConstraintModule(cs, create_map=False, wide_backward="fused").wide_backward == "fused"
    for bad in ("auto", "bogus", None, 1):
        with pytest.raises(ValueError):
            ConstraintModule(cs, create_map=False, wide_backward=bad)
    for method in ("RAYEN_old", "UU", "Bar"):
        with pytest.raises(ValueError):
            ConstraintModule(workloads.build_constraints(workloads.random_lin_quad_soc(k=3, m=7, n_quad=0, n_soc=0, seed=3)),
                             create_map=False, method=method, wide_backward="fused")
    with pytest.raises(ValueError):
        ops.backward_raw(torch.zeros(1, 5), None, None, torch.zeros(1, 5), None, wide_backward="auto")
    # the route key: the defaults keep the keys they had, every pair with the fused backward has one of its own
    assert ConstraintModule(cs, create_map=False)._route_key() is False
    assert ConstraintModule(cs, create_map=False, wide_kernel="fused")._route_key() == "fused"
    assert ConstraintModule(cs, create_map=False, wide_backward="fused")._route_key() == "products+bwd_fused"
    assert ConstraintModule(cs, create_map=False, wide_kernel="fused", wide_backward="fused")._route_key() == "fused+bwd_fused"


def test_pickles_and_host_tensors():
    cs = _small()
    layer = ConstraintModule(cs, create_map=False, wide_backward="fused")
    again = pickle.loads(pickle.dumps(layer))
    assert again.wide_backward == "fused" and again.wide_kernel == "products"
    state = layer.__getstate__()
    del state["wide_backward"]                         # a pickle from before the keyword
    old = ConstraintModule.__new__(ConstraintModule)
    old.__setstate__(state)
    assert old.wide_backward == "products" and old._route_key() is False
    # host tensors (and n = 5, far from the wide route): the keyword does nothing
    x = torch.linspace(-1, 1, 10).reshape(2, 5, 1)
    grads = []
    for m in (again, ConstraintModule(cs, create_map=False)):
        xg = x.clone().requires_grad_(True)
        y = m(xg)
        y.sum().backward()
        grads.append((y.detach(), xg.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    # n = 16 on the host likewise
    cs16 = workloads.build_constraints(workloads.make_raw("c2", seed=0))
    assert cs16.n == 16
    x = torch.empty(4, 16, 1).uniform_(-1, 1, generator=torch.Generator().manual_seed(1))
    assert torch.equal(ConstraintModule(cs16, create_map=False, wide_backward="fused")(x), ConstraintModule(cs16, create_map=False)(x))


def test_binding_and_header_declare_the_same_entry_points(tmp_path):
    text = open(os.path.join(REPO, "include", "rayen_hip_wide_fused_bwd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.EXPORTS_WIDE_FUSED_BWD)
    assert not set(declared) & set(_lib.EXPORTS) and not set(declared) & set(_lib.EXPORTS_WIDE_FUSED)
    main_header = open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    assert '#include "rayen_hip_wide_fused_bwd.h"' in main_header
    assert re.search(r"#define RAYEN_ABI_VERSION 15\b", main_header) and _lib.ABI_VERSION == 15
    assert "rayen_wide_fused_bwd.hip" in _build.SOURCES and "-fno-slp-vectorize" in _build.EXTRA_FLAGS["rayen_wide_fused_bwd.hip"]
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    # argument checks that need no device
    assert lib.rayen_wide_fused_bwd_served(None, 0) == 0 and lib.rayen_wide_fused_bwd_served(None, 1) == 0
    assert lib.rayen_wide_fused_bwd_workspace_bytes(None, 300) == 0
    assert lib.rayen_ray_project_wide_fused_bwd_f32(None, None, 0, 1, None, None, None, 1, None, 1, None, 0, None) == -1
    assert hasattr(torch.ops.rayen_amd, "ray_project_wide") and hasattr(torch.ops.rayen_amd, "ray_project_bwd_wide_fused")
    # the public header in a C99 translation unit
    src = tmp_path / "c99.c"
    src.write_text('#include "rayen_hip.h"\nint main(void) { return rayen_wide_fused_bwd_served(0, 0) != 0; }\n')
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the image"
    built = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(REPO, "include"),
                            str(src)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
