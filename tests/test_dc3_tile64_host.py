"""Host side of the fp64 DC3 tile kernels (rayen_amd/csrc/rayen_dc3_tile64.hip), no GPU: the calls
tests/test_gpu_dc3_tile64.py judges the kernels by are sound on the host reference alone (finite, no residual near a kink at
a visited step, the stop decided with 0.5 % to spare, the reference's own gap under another summation order printed and
held at 1e-13); the image header compiles alone and lays out what its comment says; the envelope rule answers from Python;
the six entry points are declared, exported and linkable from plain C and refuse bad arguments."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import dc3_reference as ref
import dc3_tile64_cases as tc
from rayen_amd import _build, _lib, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rayen_amd", "csrc")


# ------------------------------------------------------------------------------------------------ the yardstick is sound

def test_the_cases_are_what_the_fp64_lane_kernel_refuses_and_serves():
    for case in tc.BEYOND_CASES:
        assert not ref.served(case, torch.float64), case.name
    for case in tc.SMALL_CASES:
        assert ref.served(case, torch.float64), case.name
    assert tc.CASE["np32_n17_one_quadratic"].n == 17 and tc.CASE["tile_n30_corridor_shape"][1:5] == (30, 1050, 72, 15)


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_calls_are_sound(case):
    for B, limit, t_star in tc.BACKWARD_CALLS:
        call = tc.call_for(case.name, B, limit, t_star)
        gap_y, gap_g = tc.reorder_gap(call)
        print(f"{case.name} B={B} ({limit}, {t_star}): nearest residual {call.nearest:.2e}  reorder gap y {gap_y:.2e} "
              f"grad {gap_g:.2e}")
        assert tc.sound(call) == [], (case.name, B, limit, t_star)
        assert call.steps == tc.expected_steps(case, limit, t_star)
        assert gap_y <= tc.REORDER_BAR and gap_g <= tc.REORDER_BAR
    for B, limit, t_star in tc.FORWARD_CALLS:
        call = tc.forward_call_for(case.name, B, limit, t_star)
        assert tc.sound(call, backward=False) == [], (case.name, B, limit, t_star)
        assert call.steps == tc.expected_steps(case, limit, t_star)


@pytest.mark.parametrize("name", tc.POSITION_CASES)
def test_position_calls_are_sound(name):
    for limit, t_star in tc.POSITIONS:
        call = tc.call_for(name, tc.POSITION_BATCH, limit, t_star)
        assert tc.sound(call) == [], (name, limit, t_star)
        assert call.steps == t_star


def test_the_other_calls_of_the_gpu_file_are_sound():
    for name in tc.MATES_CASES:
        call = tc.call_for(name, max(tc.MATES_BATCHES), tc.MATES_STEPS, None)
        assert tc.sound(call) == [] and call.steps == tc.MATES_STEPS
    clean = tc.forward_call_for("np8_n5_ragged_everything", 33, 40, 7)
    assert tc.sound(clean, backward=False) == [] and clean.steps == 7
    for name in ("np32_n17_one_quadratic", "tile_n33_forty_quadratics"):
        assert tc.sound(tc.call_for(name, 65, 10, 7)) == []


# ------------------------------------------------------------------------------------------------ the image header

PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rayen_dc3_tile_image.h"
using Layout = rayen::Dc3TileLayout64;
static std::vector<double> take(FILE* f, size_t count) {
  std::vector<double> v(count + 1);
  if (count && fread(v.data(), sizeof(double), count, f) != count) exit(3);
  return v;
}
int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int n = atoi(argv[1]), m = atoi(argv[2]), nq = atoi(argv[3]), no = atoi(argv[4]);
  FILE* f = fopen(argv[5], "rb");
  if (!f) return 2;
  std::vector<double> A = take(f, (size_t)m * n), b = take(f, m), P = take(f, (size_t)nq * n * n), q = take(f, (size_t)nq * n),
                      r = take(f, nq), C = take(f, (size_t)no * n), c0 = take(f, no);
  fclose(f);
  std::vector<double> h;
  if (!Layout::image(n, m, nq, no, A.data(), b.data(), P.data(), q.data(), r.data(), C.data(), c0.data(), &h)) return 4;
  if ((int64_t)h.size() != Layout::dims(n, m, nq, no).total) return 5;
  if (Layout::image(65, m, nq, no, A.data(), b.data(), P.data(), q.data(), r.data(), C.data(), c0.data(), &h)) return 6;
  FILE* o = fopen(argv[6], "wb");
  if (!o || fwrite(h.data(), sizeof(double), h.size(), o) != h.size()) return 7;
  fclose(o);
  return 0;
}
"""


def test_the_image_header_compiles_alone_and_lays_out_what_it_says(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    src, exe = tmp_path / "image_probe.cc", tmp_path / "image_probe"
    src.write_text(PROBE)
    built = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    for name in ("np8_n5_ragged_everything", "np32_n17_one_quadratic"):          # n = 5, and n = 17 with ragged m
        case = tc.CASE[name]
        a = ref.make_pack(case)
        blob, out = tmp_path / (name + ".in"), tmp_path / (name + ".out")
        with open(blob, "wb") as f:
            for key in ("A1e", "b1e", "Pe", "qe", "re", "C", "c0"):
                f.write(np.ascontiguousarray(a[key], dtype=np.float64).tobytes())
        ran = subprocess.run([str(exe), *(str(x) for x in (case.n, case.m, case.nq, case.no)), str(blob), str(out)],
                             capture_output=True, text=True)
        assert ran.returncode == 0, (ran.returncode, ran.stderr)
        got = np.fromfile(out, dtype=np.float64)
        want = tc.image(a)
        assert got.shape == want.shape and np.array_equal(got, want), name
        assert np.count_nonzero(want) >= case.m * case.n * 2            # (A1e is there twice: rows and columns)


# ------------------------------------------------------------------------------------------------ the envelope, from Python

def test_shape_served_against_the_formula():
    served = _lib.load().rayen_dc3_tile64_shape_served
    for case in tc.CASES + list(ref.CASES) + list(ref.LDS_CASES):
        assert served(case.n, case.m, case.nq, case.no) == 1 == tc.shape_served(case.n, case.m, case.nq, case.no), case.name
    assert served(64, 128, 4, 0) == 1 and served(65, 128, 4, 0) == 0 and served(0, 1, 0, 0) == 0
    assert served(8, -1, 0, 0) == 0 and served(8, 0, -1, 0) == 0 and served(8, 0, 0, -1) == 0
    assert served(64, 2 ** 31 - 1, 0, 0) == 0
    # the 1 GiB edge at n = 64: a 16-row block of A1e is 8 * 128 + 4 * 256 + 16 doubles
    d = tc.dims(64, 16, 0, 0)
    assert d["total"] == 2064 + 2 and (d["nx"], d["kg"], d["kp"], d["Mb"]) == (4, 16, 8, 1)
    blocks = ((1 << 27) - 2) // 2064
    for m in (16 * blocks - 15, 16 * blocks, 16 * blocks + 1, 16 * blocks + 16):
        assert served(64, m, 0, 0) == int(tc.shape_served(64, m, 0, 0)) == int(m <= 16 * blocks), m
    for n, m, nq, no in ((1, 0, 0, 0), (17, 6, 1, 5), (33, 40, 40, 2), (64, 0, 300, 70)):
        assert served(n, m, nq, no) == int(tc.shape_served(n, m, nq, no))
    assert tc.dims(17, 6, 1, 5) == dict(nx=2, kg=5, kp=3, Mb=1, Cb=1, off_A=0, off_AT=384, off_b=896, off_P=912, off_PT=1680,
                                        off_q=2448, off_r=2480, off_C=2482, off_CT=2866, off_c0=3378, total=3396)


# ------------------------------------------------------------------------------------------------ the symbols

def _declared():
    text = open(os.path.join(REPO, "include", "rayen_hip_dc3_tile64.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))


def test_symbols_are_declared_exported_and_link_from_plain_c(tmp_path):
    declared = _declared()
    assert set(declared) == set(_lib.EXPORTS_DC3_TILE64) and len(declared) == 6
    assert not set(declared) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_TILE) | set(_lib.EXPORTS_DC3_TILE))
    main_header = open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    assert '#include "rayen_hip_dc3_tile64.h"' in main_header
    lib_path = _build.build()
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rayen_abi_version() == _lib.ABI_VERSION == 15
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    body = "\n".join(f"  table[n++] = (void (*)(void)){name};" for name in declared)
    src = tmp_path / "dc3_tile64_probe.c"
    src.write_text(f"""
#include <stdio.h>
#include "rayen_hip.h"
int main(void) {{
  void (*table[{len(declared)}])(void);
  int n = 0;
{body}
  if (rayen_abi_version() != RAYEN_ABI_VERSION || RAYEN_ABI_VERSION != 15) return 2;
  for (int i = 0; i < n; ++i) if (table[i] == NULL) return 5;
  if (rayen_dc3_tile64_shape_served(64, 128, 4, 0) != 1 || rayen_dc3_tile64_shape_served(65, 1, 0, 0) != 0) return 6;
  if (rayen_dc3_tile64_served(NULL) != 0) return 7;
  printf("%d\\n", n);
  return 0;
}}
""")
    exe = tmp_path / "dc3_tile64_probe"
    libdir = os.path.dirname(lib_path)
    cmd = [gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src),
           "-L", libdir, "-l:" + os.path.basename(lib_path), "-Wl,-rpath," + libdir, "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stdout, ran.stderr)
    assert ran.stdout.split()[0] == "6"


def test_null_and_bad_arguments():
    lib = _lib.load()
    bad = -1                                                   # RAYEN_E_BAD_ARG
    assert lib.rayen_dc3_tile64_served(None) == 0
    assert lib.rayen_dc3_tile64_workspace_bytes(None, 1, 1, 0) == -1
    assert lib.rayen_dc3_tile64_pack_set(None, None, None, None, None, None, None, None) == bad
    assert lib.rayen_dc3_tile64_forward_f64(None, None, 1, 1, None, 1, 0.0, 0.0, 0.0, 1, None, None, 0, None, None) == bad
    assert lib.rayen_dc3_tile64_backward_f64(None, None, 1, 1, None, 1, None, 1, 0.0, 0.0, 1, None, None, 0, None) == bad


# ------------------------------------------------------------------------------------------------ Python's names

ARGS = dict(lr=1e-3, momentum=0.5, eps_converge=1e-4, max_steps_training=5, max_steps_testing=7)


def test_kernel_names():
    assert ops.DC3_KERNELS == ("lane", "tile") and ops.DC3_KERNELS_F64 == ("lane", "tile64")
    assert callable(ops.dc3_tile64_served)
    assert hasattr(torch.ops.rayen_amd, "dc3_project_tile64") and hasattr(torch.ops.rayen_amd, "dc3_project_tile64_bwd")
    raw = workloads.random_lin_quad_soc(k=6, m=8, n_quad=1, n_soc=0, seed=3)
    cs = workloads.build_constraints(raw)
    layer = ConstraintModule(cs, method="DC3", create_map=False, args_DC3=dict(ARGS, kernel="tile"))
    assert layer._dc3_kernel_for(None, torch.float32) == "tile" and layer._dc3_kernel_for(None, torch.float64) == "tile64"
    for kernel in (None, "lane"):
        args = dict(ARGS) if kernel is None else dict(ARGS, kernel=kernel)
        plain = ConstraintModule(cs, method="DC3", create_map=False, args_DC3=args)
        assert plain._dc3_kernel_for(None, torch.float32) == plain._dc3_kernel_for(None, torch.float64) == "lane"
