"""Host checks of the tile kernel's surroundings (rayen_amd/csrc/rayen_proj_tile.hip): the re-laying of the rows against
its Python restatement (tests/tile_layout_formulas.py), the padded program against the original in the fp64 mirror, the
fixtures of tests/proj_tile_cases.py against the reference, and the ``kernel=`` keyword.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import proj_reference as pr                                  # noqa: E402
import proj_tile_cases as ptc                                # noqa: E402
import tile_layout_formulas as tl                            # noqa: E402
from rayen_amd import _lib, projection, workloads            # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the degenerate programs: (m_lin, soc_rows)
DEGENERATE = {"no_orthant_row": (0, [3]), "one_row": (1, []), "a_cone_of_66": (0, [66]), "72_cones_of_5": (0, [5] * 72)}
CONFIG_SHAPE = {"c3": (64, 522, 6), "c5": (30, 1410, 72)}          # (n, m, cones) of the programs of configs 3 and 5


def _program(name):
    if name in CONFIG_SHAPE:
        prog = projection.build_program(workloads.build_constraints(workloads.make_raw(name)), rho=1.0)
        assert (prog.n, prog.m, len(prog.soc_rows)) == CONFIG_SHAPE[name]
        return prog
    return pr.module_for(name).program


def _program_rows(name):
    prog = _program(name)
    return prog.m_lin, list(prog.soc_rows), prog.n


def c_layout(m_lin, soc_rows):
    lib = _lib.load()
    soc = np.asarray(soc_rows, dtype=np.int32)
    Mp = ctypes.c_int32(-1)
    perm = np.full(tl.MAX_ROWS, -7, dtype=np.int32)
    first = np.full(5, -7, dtype=np.int32)
    code = lib.rayen_proj_tile_layout(int(m_lin), soc.ctypes.data if soc.size else None, int(soc.size), ctypes.byref(Mp),
                                      perm.ctypes.data, first.ctypes.data)
    return code, Mp.value, perm[:max(Mp.value, 0)].tolist(), first.tolist()


PROGRAMS = [(name, None) for name in ptc.NAMES + ["n16_four_quadratics", "c3", "c5"]] + [(name, rows) for name, rows in DEGENERATE.items()]


@pytest.mark.parametrize("name,rows", PROGRAMS, ids=[p[0] for p in PROGRAMS])
def test_layout_against_its_restatement(name, rows):
    m_lin, soc_rows, n = _program_rows(name) if rows is None else rows + (1,)
    m = m_lin + sum(soc_rows)
    code, Mp, perm, first = c_layout(m_lin, soc_rows)
    assert code == 0
    want = tl.layout(m_lin, soc_rows)
    assert want is not None and (Mp, perm, first) == want[:3]
    # every original row exactly once, pads are -1
    assert sorted(r for r in perm if r >= 0) == list(range(m)) and all(r >= -1 for r in perm)
    # whole blocks, in order, within the envelope (the register file: 12 blocks a wave at n <= 32, 10 above)
    assert Mp == 32 * first[4] and first[0] == 0 and all(a <= b for a, b in zip(first, first[1:]))
    assert max(b - a for a, b in zip(first, first[1:])) <= tl.max_blocks(n) and Mp <= tl.MAX_ROWS
    # no cone crosses a wave's range, and a cone's rows are consecutive
    where = {r: i for i, r in enumerate(perm) if r >= 0}
    at = m_lin
    for cone in soc_rows:
        spots = [where[r] for r in range(at, at + cone)]
        assert spots == list(range(spots[0], spots[0] + cone))
        assert len({sum(1 for f in first[1:4] if s >= 32 * f) for s in spots}) == 1
        at += cone


def test_layout_refuses_what_no_wave_holds():
    assert c_layout(4 * 32 * 12 + 1, [])[0] == _lib.E_UNSUPPORTED
    assert c_layout(0, [32 * 12 + 1])[0] == _lib.E_UNSUPPORTED
    assert c_layout(10, [0])[0] != 0


@pytest.mark.parametrize("name", ptc.NAMES + ["n16_four_quadratics"])
def test_the_padded_program_is_the_original_program(name):
    prog = pr.module_for(name).program
    code, Mp, perm, first = c_layout(prog.m_lin, prog.soc_rows)          # (the library's layout, not its restatement)
    assert code == 0
    perm = np.asarray(perm)
    real = perm >= 0
    G, h = np.zeros((Mp, prog.n)), np.zeros(Mp)
    G[real], h[real] = prog.G[perm[real]], prog.h[perm[real]]
    # the padded program's cones: runs of consecutive cone rows, in padded order; everything else is an orthant row.  The
    # mirror wants orthant rows first, so it is given the rows sorted (orthant and pads, then the cones): a second
    # permutation that the check undoes.
    cone_spots = [i for i in range(Mp) if perm[i] >= prog.m_lin]
    order = np.asarray([i for i in range(Mp) if perm[i] < prog.m_lin] + cone_spots)
    cones, at = [], prog.m_lin
    by_first = {}
    for c, rows in enumerate(prog.soc_rows):
        by_first[at] = rows
        at += rows
    i = 0
    while i < len(cone_spots):
        rows = by_first[perm[cone_spots[i]]]
        cones.append(rows)
        i += rows
    padded = projection.Program(G[order], h[order], Mp - len(cone_spots), cones, prog.n, prog.rho)
    q = torch.from_numpy(pr.make_inputs(name)[0][:33])
    cpu = torch.device("cpu")
    z0, it0, v0 = projection.mirror_forward(projection.Constants(prog, torch.float64, cpu), q, pr.MAX_ITERS, 1e-9)
    z1, it1, v1 = projection.mirror_forward(projection.Constants(padded, torch.float64, cpu), q, pr.MAX_ITERS, 1e-9)
    back = np.empty(Mp, dtype=np.int64)
    back[order] = np.arange(Mp)                      # padded row -> its place in the sorted program
    v1 = v1.numpy()[:, back]
    unpermuted = np.zeros((33, prog.m))
    unpermuted[:, perm[real]] = v1[:, real]
    assert torch.equal(it0, it1)
    assert np.max(np.abs(z0.numpy() - z1.numpy())) <= 1e-12
    assert np.max(np.abs(unpermuted - v0.numpy())) <= 1e-12
    assert np.all(v1[:, ~real] == 0.0)


@pytest.mark.parametrize("name", ptc.NAMES)
def test_fixtures_are_what_the_reference_says(name):
    assert pr.shape_of(name) == ptc.SHAPE[name]
    assert not pr.served(*ptc.SHAPE[name], 4)
    ref, cs = ptc.reference(name), pr.make_cs(name)
    assert ref.z.shape == (pr.BATCH, cs.n) and ref.grad_q.shape == (pr.BATCH, cs.n)
    assert np.count_nonzero(ref.kink) <= pr.kink_cap(pr.BATCH)
    rows = np.random.default_rng(len(name)).choice(pr.BATCH, 16, replace=False)
    z = pr.project_rows(cs, ref.q[rows])
    assert np.max(np.abs(z - ref.z[rows])) <= 1e-9
    gz = ref.gy @ cs.NA_E
    for b, zb in zip(rows, z):
        J, margin = pr.jacobian_row(cs, ref.q[b], zb)
        if margin >= pr.KINK_MARGIN:
            assert np.max(np.abs(J @ gz[b] - ref.grad_q[b])) <= 1e-9 * (1.0 + np.max(np.abs(ref.grad_q[b])))
    # the recorded fp32 mirror passes the comparisons every kernel faces
    run = ptc.mirror_run(name)
    assert ptc.compare(name, run.z, run.grad_q, run.iters) == []


def _tile_header_symbols():
    text = open(os.path.join(REPO, "include", "rayen_hip_tile.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))


def test_the_tile_header_is_the_binding_and_links_from_c(tmp_path):
    """include/rayen_hip_tile.h (part of rayen_hip.h) against ``_lib.EXPORTS_TILE`` and the library, and from plain C: what
    tests/test_abi_load.py does for the entry points rayen_hip.h declares itself."""
    import shutil
    import subprocess
    declared = _tile_header_symbols()
    assert set(declared) == set(_lib.EXPORTS_TILE) and len(declared) == 5
    assert not set(declared) & set(_lib.EXPORTS)
    main_header = open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    assert '#include "rayen_hip_tile.h"' in main_header
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rayen_abi_version() == _lib.ABI_VERSION == 15
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    lib_path = _lib.library_path()
    body = "\n".join(f"  table[n++] = (void (*)(void)){name};" for name in declared)
    src = tmp_path / "tile_probe.c"
    src.write_text(f"""
#include <stdio.h>
#include "rayen_hip.h"
int main(void) {{
  void (*table[{len(declared)}])(void);
  int n = 0;
  int32_t cones[2] = {{5, 5}}, Mp = -1, first[5], perm[128 * 12];
{body}
  for (int i = 0; i < n; ++i) if (table[i] == NULL) return 5;
  if (rayen_proj_tile_layout(40, cones, 2, &Mp, perm, first) != RAYEN_OK) return 6;
  if (Mp != 96 || first[4] != 3 || perm[0] != 40 || perm[10] != -1 || perm[32] != 0) return 7;
  if (rayen_proj_tile_served(NULL) != 0) return 8;
  printf("%d %d\\n", n, (int)Mp);
  return 0;
}}
""")
    exe = tmp_path / "tile_probe"
    libdir = os.path.dirname(lib_path)
    cmd = [gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src),
           "-L", libdir, "-l:" + os.path.basename(lib_path), "-Wl,-rpath," + libdir, "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stdout, ran.stderr)
    assert ran.stdout.split() == ["5", "96"]


def test_a_module_pickled_before_the_keyword_runs_the_wave_kernel():
    import pickle
    layer = projection.ProjectionModule(pr.make_cs("n3_box"), create_map=False)
    state = layer.__getstate__()
    state.pop("kernel")
    state.pop("_auto_kernel")
    old = projection.ProjectionModule.__new__(projection.ProjectionModule)
    old.__dict__.update(pickle.loads(pickle.dumps(state)))
    q = torch.from_numpy(pr.make_inputs("n3_box")[0][:9]).float()
    z, iters = old.project(q)
    zn, itn = layer.project(q)
    assert torch.equal(z, zn) and torch.equal(iters, itn)


def test_the_kernel_keyword():
    cs = pr.make_cs("k8_n5_ragged_equalities")
    with pytest.raises(ValueError):
        projection.ProjectionModule(cs, create_map=False, kernel="bogus")
    assert projection.ProjectionModule(cs, create_map=False).kernel == "wave"
    layer = projection.ProjectionModule(cs, create_map=False, kernel="tile")
    with pytest.raises(ValueError):
        layer.project(torch.zeros(1, cs.n), kernel="bogus")
    q = torch.from_numpy(pr.make_inputs("k8_n5_ragged_equalities")[0][:17]).float()
    z, iters = layer.project(q)
    c = layer.constants(torch.float32, torch.device("cpu"))
    zm, im, _ = projection.mirror_forward(c, q, layer.max_iters, layer.eps)
    assert torch.equal(z, zm) and torch.equal(iters, im)
    yb, _ = cs.projectBatch(q @ torch.from_numpy(cs.NA_E.T).float() + torch.from_numpy(cs.yp.T).float(), kernel="tile")
    assert yb.shape == (17, cs.k)
