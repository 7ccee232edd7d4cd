"""Host checks of the fp64 tile kernel's surroundings (rayen_amd/csrc/rayen_proj_tile64.hip): the re-laying of the rows, the
envelope and the LDS bytes (rayen_proj_tile64_layout.h) against their Python restatement (tests/tile64_layout_formulas.py),
the padded program against the original in the fp64 mirror, the recorded fp64 mirror runs against the comparisons every
kernel faces, and include/rayen_hip_tile64.h from plain C.  No GPU."""
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
import proj_tile64_cases as p64                              # noqa: E402
import tile64_layout_formulas as tl                          # noqa: E402
from rayen_amd import _lib, projection, workloads            # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, m_lin, soc_rows): rows about one and two blocks, a cone that ends exactly on a block edge and one that ends one past
# it, and the degenerate programs of tests/test_proj_tile_host.py
EDGES = {"rows_15": (3, 15, []), "rows_16": (3, 16, []), "rows_17": (3, 17, []), "rows_31": (3, 31, []),
         "rows_32": (3, 32, []), "rows_33": (3, 33, []), "cone_ends_on_the_edge": (4, 5, [16]),
         "cone_ends_one_past_the_edge": (4, 5, [17]), "two_cones_fill_a_block": (4, 5, [7, 9, 3]),
         "no_orthant_row": (1, 0, [3]), "one_row": (1, 1, []), "a_cone_of_66": (1, 0, [66]), "72_cones_of_5": (1, 0, [5] * 72),
         "largest_n32": (32, tl.MAX_ROWS, []), "largest_n64": (64, 4 * 16 * 20, []), "n_40_twenty_blocks": (40, 1264, [9])}
CONFIG_SHAPE = {"c3": (64, 522, 6), "c5": (30, 1410, 72)}          # (n, m, cones) of the programs of configs 3 and 5


def _program(name):
    if name in CONFIG_SHAPE:
        prog = projection.build_program(workloads.build_constraints(workloads.make_raw(name)), rho=1.0)
        assert (prog.n, prog.m, len(prog.soc_rows)) == CONFIG_SHAPE[name]
        return prog
    return pr.module_for(name).program


def c_layout(n, m_lin, soc_rows):
    lib = _lib.load()
    soc = np.asarray(soc_rows, dtype=np.int32)
    Mp, lds = ctypes.c_int32(-1), ctypes.c_int64(-1)
    perm = np.full(tl.MAX_ROWS, -7, dtype=np.int32)
    first = np.full(5, -7, dtype=np.int32)
    code = lib.rayen_proj_tile64_layout(int(n), int(m_lin), soc.ctypes.data if soc.size else None, int(soc.size),
                                        ctypes.byref(Mp), perm.ctypes.data, first.ctypes.data, ctypes.byref(lds))
    return code, Mp.value, perm[:max(Mp.value, 0)].tolist(), first.tolist(), lds.value


PROGRAMS = [(name, None) for name in list(pr.SHAPE) + list(ptc.SHAPE) + ["c5"]] + list(EDGES.items())


@pytest.mark.parametrize("name,rows", PROGRAMS, ids=[p[0] for p in PROGRAMS])
def test_layout_against_its_restatement(name, rows):
    if rows is None:
        prog = _program(name)
        n, m_lin, soc_rows = prog.n, prog.m_lin, list(prog.soc_rows)
        if name in pr.SHAPE or name in ptc.SHAPE:
            assert (prog.n, prog.m, len(prog.soc_rows)) == {**pr.SHAPE, **ptc.SHAPE}[name]
    else:
        n, m_lin, soc_rows = rows
    m = m_lin + sum(soc_rows)
    code, Mp, perm, first, lds = c_layout(n, m_lin, soc_rows)
    assert code == 0 and tl.served(n, m_lin, soc_rows)
    want = tl.layout(m_lin, soc_rows, tl.max_blocks(n))
    assert want is not None and (Mp, perm, first) == want[:3]
    assert lds == tl.lds_bytes(n, m_lin, soc_rows) <= tl.LDS_LIMIT
    # every original row exactly once, pads are -1
    assert sorted(r for r in perm if r >= 0) == list(range(m)) and all(r >= -1 for r in perm)
    # whole blocks, in order, within the envelope (the register file: 24 blocks a wave at n <= 32, 20 above)
    assert Mp == 16 * first[4] and first[0] == 0 and all(a <= b for a, b in zip(first, first[1:]))
    assert max(b - a for a, b in zip(first, first[1:])) <= want[3] <= tl.max_blocks(n) and Mp <= tl.MAX_ROWS
    # no cone crosses a wave's range, a cone's rows are consecutive, a wave's cones come before its orthant rows
    where = {r: i for i, r in enumerate(perm) if r >= 0}
    at = m_lin
    for cone in soc_rows:
        spots = [where[r] for r in range(at, at + cone)]
        assert spots == list(range(spots[0], spots[0] + cone))
        wave = {sum(1 for f in first[1:4] if s >= 16 * f) for s in spots}
        assert len(wave) == 1
        w = wave.pop()
        assert all(perm[i] < 0 or perm[i] >= m_lin for i in range(16 * first[w], spots[0]))
        at += cone


def test_the_benchmark_shapes_are_served_within_lds():
    for name, lds_cap in (("n64_c3_shape", tl.LDS_LIMIT), ("c5", tl.LDS_LIMIT)):
        prog = _program(name)
        code, Mp, perm, first, lds = c_layout(prog.n, prog.m_lin, prog.soc_rows)
        NB, NX = tl.instance(max(b - a for a, b in zip(first, first[1:])), prog.n)
        print(f"{name}: (n, m, cones) = {(prog.n, prog.m, len(prog.soc_rows))} Mp {Mp} blocks {first} instance {(NB, NX)} "
              f"backward LDS {lds} forward LDS {tl.lds_bytes(prog.n, prog.m_lin, prog.soc_rows, False)}")
        assert code == 0 and 0 < lds <= lds_cap == 160 * 1024 - 256
    assert tl.instance(tl.layout(_program("c5").m_lin, _program("c5").soc_rows)[3], 30) == (24, 2)


def test_layout_refuses_what_is_outside_the_envelope():
    assert c_layout(8, tl.MAX_ROWS + 1, [])[0] == _lib.E_UNSUPPORTED and not tl.served(8, tl.MAX_ROWS + 1, [])
    assert c_layout(8, tl.MAX_ROWS, [])[0] == 0
    assert c_layout(33, 4 * 16 * 20 + 1, [])[0] == _lib.E_UNSUPPORTED and not tl.served(33, 4 * 16 * 20 + 1, [])
    assert c_layout(8, 0, [16 * 24 + 1])[0] == _lib.E_UNSUPPORTED and not tl.served(8, 0, [16 * 24 + 1])
    assert c_layout(65, 10, [])[0] == _lib.E_UNSUPPORTED and not tl.served(65, 10, [])
    assert c_layout(64, 10, [])[0] == 0
    # the backward holds the cone blocks' images twice: cones alone can be over LDS
    assert c_layout(8, 0, [300] * 4)[0] == _lib.E_UNSUPPORTED and not tl.served(8, 0, [300] * 4)
    assert c_layout(8, 10, [0])[0] not in (0, _lib.E_UNSUPPORTED)
    assert c_layout(0, 10, [])[0] not in (0, _lib.E_UNSUPPORTED)


@pytest.mark.parametrize("name", ptc.NAMES + ["n16_four_quadratics", "k8_n5_ragged_equalities"])
def test_the_padded_program_is_the_original_program(name):
    prog = pr.module_for(name).program
    code, Mp, perm, first, _ = c_layout(prog.n, prog.m_lin, prog.soc_rows)      # (the library's layout, not its restatement)
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
    cones, at, by_first = [], prog.m_lin, {}
    for rows in prog.soc_rows:
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


@pytest.mark.parametrize("name", p64.RECORDED)
def test_the_recorded_fp64_mirror_passes_what_the_kernel_faces(name):
    run, ref = p64.host_mirror(name), p64.reference(name)
    assert run.z.shape == ref.z.shape == (p64.rows_of(name), pr.module_for(name).program.n)
    assert int(run.iters.max()) < pr.MAX_ITERS
    assert p64.compare(name, run.z, run.grad_q, run.iters) == []
    rows = np.random.default_rng(len(name)).choice(p64.rows_of(name), 5, replace=False)
    c = pr.module_for(name).constants(torch.float64, torch.device("cpu"))
    z, iters, _ = projection.mirror_forward(c, torch.from_numpy(ref.q[rows]), pr.MAX_ITERS, pr.EPS[p64.F64])
    assert np.array_equal(iters.numpy(), run.iters[rows]) and np.max(np.abs(z.numpy() - run.z[rows])) <= 1e-12


def _header_symbols():
    text = open(os.path.join(REPO, "include", "rayen_hip_tile64.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))


def test_the_tile64_header_is_the_binding_and_links_from_c(tmp_path):
    import shutil
    import subprocess
    declared = _header_symbols()
    assert set(declared) == set(_lib.EXPORTS_TILE64) and len(declared) == 6
    assert not set(declared) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_TILE))
    assert '#include "rayen_hip_tile64.h"' in open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rayen_abi_version() == _lib.ABI_VERSION == 15
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    lib_path = _lib.library_path()
    body = "\n".join(f"  table[n++] = (void (*)(void)){name};" for name in declared)
    src = tmp_path / "tile64_probe.c"
    src.write_text(f"""
#include <stdio.h>
#include "rayen_hip.h"
int main(void) {{
  void (*table[{len(declared)}])(void);
  int n = 0;
  int32_t cones[2] = {{5, 5}}, Mp = -1, first[5], perm[1536];
  int64_t lds = -1;
{body}
  for (int i = 0; i < n; ++i) if (table[i] == NULL) return 5;
  if (rayen_proj_tile64_layout(8, 40, cones, 2, &Mp, perm, first, &lds) != RAYEN_OK) return 6;
  if (Mp != 64 || first[4] != 4 || perm[0] != 40 || perm[10] != -1 || perm[16] != 0 || lds <= 0) return 7;
  if (rayen_proj_tile64_layout(65, 40, cones, 2, &Mp, NULL, NULL, NULL) != RAYEN_E_UNSUPPORTED) return 8;
  if (rayen_proj_tile64_served(NULL) != 0 || rayen_proj_tile64_workspace_bytes(NULL, 1, 0) != -1) return 9;
  printf("%d %d\\n", n, (int)Mp);
  return 0;
}}
""")
    exe = tmp_path / "tile64_probe"
    libdir = os.path.dirname(lib_path)
    cmd = [gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src),
           "-L", libdir, "-l:" + os.path.basename(lib_path), "-Wl,-rpath," + libdir, "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stdout, ran.stderr)
    assert ran.stdout.split() == ["6", "64"]


def test_the_kernel_names():
    from rayen_amd import ops
    assert ops.PROJ_KERNELS == ("wave", "tile") and ops.PROJ_KERNELS_F64 == ("wave", "tile64")
    assert projection.ProjectionModule.KERNELS == ("wave", "tile", "auto")
    cs = pr.make_cs("k8_n5_ragged_equalities")
    layer = projection.ProjectionModule(cs, create_map=False, kernel="tile")
    q = torch.from_numpy(pr.make_inputs("k8_n5_ragged_equalities")[0][:17])          # fp64 on the host: the mirror, as before
    z, iters = layer.project(q)
    zm, im, _ = projection.mirror_forward(layer.constants(torch.float64, torch.device("cpu")), q, layer.max_iters, layer.eps)
    assert torch.equal(z, zm) and torch.equal(iters, im)
