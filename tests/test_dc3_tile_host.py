"""Host side of the DC3 tile kernels (rayen_amd/csrc/rayen_dc3_tile.hip), no GPU: the calls tests/test_gpu_dc3_tile.py
judges the kernels by are sound on the host reference alone (finite, stop decided with 0.5 % to spare, fp32 and fp64 take
the same number of steps, rows left out by the widened kink rule within the cap); the envelope rule answers from Python; the
new entry points are declared, exported and linkable from plain C; ``args_DC3['kernel']`` is validated."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import dc3_reference as ref
import dc3_tile_cases as tc
from rayen_amd import _build, _lib, dc3, workloads
from rayen_amd.constraint_module import ConstraintModule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the yardstick is sound

def test_the_new_cases_are_beyond_the_lane_kernel():
    for case in tc.TILE_CASES:
        assert not ref.served(case, torch.float32), case.name
        assert ref.lds_bytes(case, 4) > ref.LDS_LIMIT
    assert tc.TILE_CASE["tile_n30_corridor_shape"][1:5] == tc.CORRIDOR_SHAPE


@pytest.mark.parametrize("case", tc.TILE_CASES, ids=lambda c: c.name)
def test_new_case_calls_are_sound(case):
    for B, limit, t_star in tc.BACKWARD_CALLS:
        call = tc.call_for(case.name, B, limit, t_star)
        gap_y, gap_g = ref.gaps(call)
        print(f"{case.name} B={B} ({limit}, {t_star}): F {tc.largest_gap(call):.2e} kinks {int(call.kinks.sum())} "
              f"host gaps y {gap_y:.2e} grad {gap_g:.2e}")
        assert tc.sound(call) == [], (case.name, B, limit, t_star)
        assert call.steps == t_star
        assert gap_y <= 5e-7 and gap_g <= 1.4e-6
    for B, limit, t_star in tc.FORWARD_CALLS:
        call = tc.forward_call_for(case.name, B, limit, t_star)
        assert tc.sound(call, backward=False) == [], (case.name, B, limit, t_star)
        assert call.steps == (limit if t_star is None else t_star)


@pytest.mark.parametrize("case", tc.sweep_cases(), ids=lambda c: c.name)
def test_sweep_calls_stay_within_the_cap_under_the_widened_rule(case):
    for B in ref.SWEEP_BATCHES:
        for position in (ref.TRAIN_CALL, ref.EVAL_CALL):
            call = tc.call_for(case.name, B, *position)
            assert tc.sound(call) == [], (case.name, B, position)


@pytest.mark.parametrize("name", ref.POSITION_CASES)
def test_position_calls_stay_within_the_cap_under_the_widened_rule(name):
    for limit, t_star in ref.POSITIONS:
        call = tc.call_for(name, ref.POSITION_BATCH, limit, t_star)
        assert tc.sound(call) == [], (name, limit, t_star)
        assert call.steps == (limit if t_star is None else t_star)


def test_the_other_calls_of_the_gpu_file_are_sound():
    for B in tc.OUTLIER_BATCHES:
        far, near = tc.outlier_calls(B)
        assert tc.sound(far) == [] and tc.sound(near) == []
        assert near.steps == 1 < far.steps == ref.OUTLIER_CALL[1]
    for name in tc.MATES_CASES:
        call = tc.call_for(name, 257, 10, None)
        assert tc.sound(call) == [] and call.steps == 10
    for limit, t_star in (ref.TRAIN_CALL, ref.EVAL_CALL):
        assert tc.sound(tc.call_for("np32_n32_full", 65, limit, t_star)) == []
    clean = tc.forward_call_for("np8_n5_ragged_everything", 33, 40, 7)
    assert tc.sound(clean, backward=False) == [] and clean.steps == 7


# ------------------------------------------------------------------------------------------------ the envelope, from Python

def test_shape_served():
    served = _lib.load().rayen_dc3_tile_shape_served
    for case in tc.TILE_CASES + list(ref.CASES) + list(ref.LDS_CASES):
        assert served(case.n, case.m, case.nq, case.no) == 1, case.name
    assert served(*tc.CORRIDOR_SHAPE) == 1
    assert served(0, 1, 0, 0) == 0 and served(65, 1, 0, 0) == 0
    assert served(8, -1, 0, 0) == 0 and served(8, 0, -1, 0) == 0 and served(8, 0, 0, -1) == 0
    assert served(64, 2 ** 31 - 1, 0, 0) == 0                   # an image beyond 1 GiB


# ------------------------------------------------------------------------------------------------ the symbols

def _declared():
    text = open(os.path.join(REPO, "include", "rayen_hip_dc3_tile.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))


def test_symbols_are_declared_exported_and_link_from_plain_c(tmp_path):
    """include/rayen_hip_dc3_tile.h (part of rayen_hip.h) against ``_lib.EXPORTS_DC3_TILE`` and the library, and from plain
    C as tests/test_abi_load.py does it for rayen_hip.h's own text."""
    declared = _declared()
    assert set(declared) == set(_lib.EXPORTS_DC3_TILE) and len(declared) == 6
    assert not set(declared) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_TILE))
    main_header = open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    assert '#include "rayen_hip_dc3_tile.h"' in main_header
    lib_path = _build.build()
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rayen_abi_version() == _lib.ABI_VERSION == 15
    assert lib.rayen_dc3_tile_served(None) == 0
    assert lib.rayen_dc3_tile_workspace_bytes(None, 1, 1, 0) == -1
    assert lib.rayen_dc3_tile_pack_set(None, None, None, None, None, None, None, None) == -1
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    body = "\n".join(f"  table[n++] = (void (*)(void)){name};" for name in declared)
    src = tmp_path / "dc3_tile_probe.c"
    src.write_text(f"""
#include <stdio.h>
#include "rayen_hip.h"
int main(void) {{
  void (*table[{len(declared)}])(void);
  int n = 0;
{body}
  if (rayen_abi_version() != RAYEN_ABI_VERSION || RAYEN_ABI_VERSION != 15) return 2;
  for (int i = 0; i < n; ++i) if (table[i] == NULL) return 5;
  if (rayen_dc3_tile_shape_served(30, 1050, 72, 15) != 1 || rayen_dc3_tile_shape_served(65, 1, 0, 0) != 0) return 6;
  if (rayen_dc3_tile_served(NULL) != 0) return 7;
  printf("%d\\n", n);
  return 0;
}}
""")
    exe = tmp_path / "dc3_tile_probe"
    libdir = os.path.dirname(lib_path)
    cmd = [gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src),
           "-L", libdir, "-l:" + os.path.basename(lib_path), "-Wl,-rpath," + libdir, "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stdout, ran.stderr)
    assert ran.stdout.split()[0] == "6"


# ------------------------------------------------------------------------------------------------ args_DC3['kernel']

ARGS = dict(lr=1e-3, momentum=0.5, eps_converge=1e-4, max_steps_training=5, max_steps_testing=7)


def test_check_args_takes_the_kernel_key():
    dc3.check_args(dict(ARGS))
    for kernel in ("lane", "tile", "auto"):
        dc3.check_args(dict(ARGS, kernel=kernel))
    assert dc3.KERNEL_CHOICES == ("lane", "tile", "auto")
    for bad in ("wave", "", None, 1):
        with pytest.raises(ValueError, match="kernel"):
            dc3.check_args(dict(ARGS, kernel=bad))


def test_a_module_reports_the_kernel_it_was_asked_for():
    raw = workloads.random_lin_quad_soc(k=6, m=8, n_quad=1, n_soc=0, seed=3)
    cs = workloads.build_constraints(raw)
    assert ConstraintModule(cs, method="DC3", create_map=False, args_DC3=dict(ARGS)).dc3_kernel == "lane"
    for kernel in ("lane", "tile", "auto"):
        assert ConstraintModule(cs, method="DC3", create_map=False, args_DC3=dict(ARGS, kernel=kernel)).dc3_kernel == kernel
    with pytest.raises(ValueError, match="kernel"):
        ConstraintModule(cs, method="DC3", create_map=False, args_DC3=dict(ARGS, kernel="wave"))
    # host tensors take the reference's formula whatever the key says
    layer = ConstraintModule(cs, method="DC3", create_map=False, args_DC3=dict(ARGS, kernel="tile")).eval()
    plain = ConstraintModule(cs, method="DC3", create_map=False, args_DC3=dict(ARGS)).eval()
    q = 0.25 * torch.randn(9, layer.dim_after_map, 1, generator=torch.Generator().manual_seed(1))
    assert torch.equal(layer(q), plain(q))
    assert np.array_equal(layer.dc3_steps.numpy(), plain.dc3_steps.numpy())
