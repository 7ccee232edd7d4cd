"""The fp64 tile soft cost without a device: rayen_amd/csrc/rayen_cost_tile64_layout.h (compiled alone with g++) against its
Python restatement (tests/cost_tile64_cases.py) and the properties it promises; the lane / register claim the kernel rests on,
on a numpy emulation of the operand and accumulator maps of v_mfma_f64_16x16x4_f64; the binding against the header; and the
``kernel='tile64'`` keyword on host tensors."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cost_cases                                             # noqa: E402
import cost_stream_cases as S                                 # noqa: E402
import cost_sweep_cases as sweep                              # noqa: E402
import cost_tile64_cases as T                                 # noqa: E402
from rayen_amd import _build, _lib, ops                       # noqa: E402
from rayen_amd.cost_computer import CostComputer              # noqa: E402
from rayen_amd.soft_cost import KERNELS, SoftCost             # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_item_lists():
    """Seeded random sets as item lists: runs at either end, quadratics and cones of 1 .. 9 blocks between."""
    rng = np.random.default_rng(1300)
    for _ in range(40):
        its = [(int(rng.integers(1, 200)), 0, 1)] if rng.random() < 0.8 else []
        for _ in range(int(rng.integers(0, 30))):
            its.append((int(rng.integers(1, 10)), 1, 0))
        if rng.random() < 0.6:
            its.append((int(rng.integers(1, 40)), 0, 1))
        if its:
            yield its, int(rng.choice([8, 16, 32, 64]))


def _jobs():
    """(what, K, window, items) of every cut the probe makes; window is what the header is handed (never 0)."""
    sets = {name: S.beyond_case(name).arrays for name in ("corridor_k12", "c5_shape", "c3", "past_limit64")}
    sets.update({f"tile_{n}": sweep.tile_set(n) for n in sweep.TILE_SETS})
    sets.update({f"block_{n}": T.boundary_case(n).arrays for n in T.BOUNDARY})
    sets["k8_windows"] = T.k8_case().arrays
    for name, a in sets.items():
        K, its = T.width(a["k"]), T.items(a)
        for window in T.forced_windows(a):
            yield name, K, window or T.DEFAULT_WINDOW, its
        yield name, K, T.smallest_window(a) - 16, its
    for j, (its, K) in enumerate(_random_item_lists()):
        largest = max(T.bytes_of(1 if s else nb, f, K) for nb, f, s in its)
        for window in (largest, largest + 16 * int(np.random.default_rng(j).integers(1, 400)), T.DEFAULT_WINDOW):
            yield f"random{j}", K, min(window, T.DEFAULT_WINDOW), its


def _run_probe(tmp_path, jobs):
    blocks = []
    for j, (_, K, window, its) in enumerate(jobs):
        rows = ", ".join(f"{{{u}, {f}, {s}}}" for u, f, s in its)
        blocks.append(f"  {{ static const rayen::CostTile64Item items[] = {{{rows}}};\n"
                      f"    cut({j}, items, {len(its)}, {K}, {window}ll); }}")
    src = tmp_path / "tile64_probe.cpp"
    src.write_text("""
#include <cstdio>
#include <vector>
#include "rayen_cost_tile64_layout.h"
static void cut(int job, const rayen::CostTile64Item* items, long long n, int K, long long window) {
  int64_t np = 0, total = 0;
  const int64_t nw = rayen::cost_tile64_partition(items, n, K, window, nullptr, 0, nullptr, 0, &np, &total);
  std::printf("job %d %lld %lld %lld\\n", job, (long long)nw, (long long)(nw < 0 ? 0 : np), (long long)(nw < 0 ? 0 : total));
  if (nw < 0) return;
  std::vector<rayen::CostTile64Window> w((size_t)nw);
  std::vector<rayen::CostTile64Piece> p((size_t)np);
  if (rayen::cost_tile64_partition(items, n, K, window, w.data(), nw, p.data(), np, nullptr, nullptr) != nw) std::printf("DRIFT\\n");
  for (const auto& x : w) {
    std::printf("w %d %d %d %d %lld :", x.piece0, x.pieces, x.blocks, x.forms, (long long)x.bytes);
    for (int i = 0; i < x.pieces; ++i) std::printf(" %d,%d,%d", p[x.piece0 + i].item, p[x.piece0 + i].block0, p[x.piece0 + i].blocks);
    std::printf("\\n");
  }
}
int main() {
  std::printf("consts %lld %lld %d %d %d %d %d\\n", (long long)rayen::kCostTile64Window, (long long)rayen::kCostTile64MaxImage,
              rayen::kCostTile64Rows, (int)rayen::cost_tile64_window_ok(0), (int)rayen::cost_tile64_window_ok(24),
              (int)rayen::cost_tile64_window_ok(rayen::kCostTile64Window + 16), (int)rayen::cost_tile64_window_ok(-16));
  std::printf("widths");
  for (int k = 0; k <= 66; ++k) std::printf(" %d", rayen::cost_tile64_width(k));
  std::printf("\\nslots");
  for (int m = 0; m < 16; ++m)
    for (int c = 0; c < 64; ++c) std::printf(" %d", rayen::cost_tile64_slot(m, c));
  std::printf("\\n");
  { static const rayen::CostTile64Item one[] = {{3, 0, 1}, {4, 1, 0}};
    std::printf("served %d %d %d %d %d\\n", (int)rayen::cost_tile64_served(64, one, 2, 0), (int)rayen::cost_tile64_served(65, one, 2, 0),
                (int)rayen::cost_tile64_served(0, one, 2, 0), (int)rayen::cost_tile64_served(64, one, 2, 1024),
                (int)rayen::cost_tile64_served(64, one, 0, 0)); }
""" + "\n".join(blocks) + "\n  return 0;\n}\n")
    exe = tmp_path / "tile64_probe"
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    built = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", _build.CSRC, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stderr)
    assert "DRIFT" not in ran.stdout
    lines = ran.stdout.strip().splitlines()
    assert lines[0].split() == ["consts", str(T.DEFAULT_WINDOW), str(T.MAX_IMAGE), str(T.ROWS), "1", "0", "0", "0"]
    assert [int(x) for x in lines[1].split()[1:]] == [T.width(k) for k in range(67)]
    assert [int(x) for x in lines[2].split()[1:]] == [T.slot(m, c) for m in range(16) for c in range(64)]
    # k = 64 served; k = 65, k = 0, a window below a quadratic of four blocks at K = 64 and a set of no items are not
    assert lines[3].split() == ["served", "1", "0", "0", "0", "0"]
    got, cur = {}, None
    for line in lines[4:]:
        f = line.split()
        if f[0] == "job":
            cur = got[int(f[1])] = dict(nw=int(f[2]), np=int(f[3]), total=int(f[4]), windows=[])
        else:
            pieces = [tuple(int(x) for x in piece.split(",")) for piece in f[7:]]
            cur["windows"].append(dict(piece0=int(f[1]), pieces=pieces, blocks=int(f[3]), forms=int(f[4]), bytes=int(f[5])))
            assert int(f[2]) == len(pieces)
    return got


def test_layout_header_matches_the_restatement_and_keeps_its_promises(tmp_path):
    jobs = list(_jobs())
    got = _run_probe(tmp_path, jobs)
    assert len(got) == len(jobs)
    split_somewhere = several = refused = 0
    for j, (name, K, window, its) in enumerate(jobs):
        what = f"{name} K {K} window {window}"
        want = T.partition(its, K, window)
        g = got[j]
        if want is None:
            assert g["nw"] == -1, what
            refused += 1
            continue
        assert g["nw"] == len(want) == len(g["windows"]), what
        assert [w["pieces"] for w in g["windows"]] == want, what
        # every block exactly once and in the stacked order; no quadratic or cone split; every window within its limit
        flat = [p for w in g["windows"] for p in w["pieces"]]
        assert g["np"] == len(flat), what
        at, order = {}, []
        for item, block0, nb in flat:
            assert nb > 0 and block0 == at.get(item, 0), what
            at[item] = block0 + nb
            if not its[item][2]:
                assert (block0, nb) == (0, its[item][0]), what + ": an item was split"
            order.append(item)
        assert order == sorted(order) and at == {i: it[0] for i, it in enumerate(its)}, what
        piece0 = 0
        for w in g["windows"]:
            assert w["piece0"] == piece0 and w["blocks"] == sum(n for _, _, n in w["pieces"]), what
            assert w["forms"] == sum(its[i][1] for i, _, _ in w["pieces"]), what
            assert w["bytes"] == T.window_bytes_of(w["pieces"], its, K) <= window and w["bytes"] % 16 == 0, what
            piece0 += len(w["pieces"])
        assert g["total"] == sum(w["bytes"] for w in g["windows"]), what
        # greedy: a window closes only when the next block (or whole item) does not fit
        for w, nxt in zip(g["windows"], g["windows"][1:]):
            item, block0, _ = nxt["pieces"][0]
            more = 1 if its[item][2] else its[item][0]
            grown = w["pieces"] + [(item, block0, more)]
            assert T.window_bytes_of(grown, its, K) > window, what + ": a window closed early without need"
        several += g["nw"] > 1
        split_somewhere += any(its[i][2] and (b0, n) != (0, its[i][0]) for i, b0, n in flat)
    assert split_somewhere and several and refused          # the cases reach every branch


def test_slot_is_a_bijection_without_bank_conflicts_for_both_products():
    """A ds_read_b64 is served per half wave on 32 words of 8 bytes: the 32 lanes of a half must read 32 different words
    modulo 32, in the first product (lane = m + 16 g reads (m, 4 j + g)) and in the second (lane = c' + 16 g reads
    (4 i + g, 16 kb + c'))."""
    for K in (8, 16, 32, 64):
        cols = range(K)
        words = sorted(T.slot(m, c) for m in range(16) for c in cols)
        assert words == list(range(16 * K)), K          # every word of the block exactly once
        for half in (0, 1):
            groups = (2 * half, 2 * half + 1)
            for j in range(K // 4):
                banks = {T.slot(m, 4 * j + g) % 32 for g in groups for m in range(16)}
                assert len(banks) == 32, (K, "first", j, half)
            for i in range(4):
                for kb in range(max(K // 16, 1)):
                    lanes = [(4 * i + g, 16 * kb + c) for g in groups for c in range(16) if 16 * kb + c < K]
                    banks = [T.slot(m, c) % 32 for m, c in lanes]
                    assert len(set(banks)) == len(banks), (K, "second", i, kb, half)


@pytest.mark.parametrize("K", [8, 16, 32, 64])
def test_in_place_coefficients_feed_the_second_product_and_Py_lines_up_with_y(K):
    """The claim the kernel rests on, on the emulated lane map.  Lane (n = lane & 15, g = lane >> 4) holds
    yv[j] = y[n][4 j + g].  First product (step j: A = W[m][4 j + g] from lane (m, g), B = yv[j]): accumulator register i of
    that lane is row 4 i + g of the block.  Coefficients written over those registers feed the second product as they lie
    (step i: A = W[4 i + g][16 kb + c'] from lane (c', g), B = register i): its accumulator register i' is column
    16 kb + 4 i' + g of the gradient -- the column of yv[4 kb + i'].  And for a block b of a quadratic's P the register i is
    (P y)[16 b + 4 i + g]: the row index of yv[4 b + i]."""
    rng = np.random.default_rng(K)
    lanes = np.arange(64)
    n, g = lanes & 15, lanes >> 4
    W = rng.standard_normal((16, K))
    Y = rng.standard_normal((16, K))          # 16 samples
    yv = [Y[n, 4 * j + g] for j in range(K // 4)]
    acc = np.zeros((64, 4))
    for j in range(K // 4):
        acc = T.mfma(W[n, 4 * j + g], yv[j], acc)          # (lane (m, g) of the A operand: m = lane & 15)
    want = W @ Y.T          # [row][sample]
    for i in range(4):
        np.testing.assert_allclose(acc[:, i], want[4 * i + g, n], rtol=1e-13, atol=1e-13)
    # coefficients in place: any function of the lane's own registers, here an odd one
    coef = np.tanh(acc)
    C = np.tanh(want)          # [row][sample]
    grad_want = C.T @ W          # [sample][column]
    for kb in range(max(K // 16, 1)):
        gacc = np.zeros((64, 4))
        for i in range(4):
            col = 16 * kb + n
            a = np.where(col < K, W[4 * i + g, np.minimum(col, K - 1)], 0.0)
            gacc = T.mfma(a, coef[:, i], gacc)
        for i2 in range(4):
            col = 16 * kb + 4 * i2 + g
            live = col < K
            np.testing.assert_allclose(gacc[live, i2], grad_want[n[live], col[live]], rtol=1e-12, atol=1e-12)
            assert np.array_equal(col[live], (4 * (4 * kb + i2) + g)[live])          # the column of yv[4 kb + i2]
    # a quadratic: blocks of 16 rows of a symmetric P (k = K); register i of block b beside yv[4 b + i]
    P = rng.standard_normal((K, K))
    P = 0.5 * (P + P.T)
    Py = Y @ P          # [sample][row]
    quad = np.zeros(64)
    for b in range(max(K // 16, 1)):
        rows = min(16, K - 16 * b)
        Wb = np.zeros((16, K))
        Wb[:rows] = P[16 * b:16 * b + rows]
        acc = np.zeros((64, 4))
        for j in range(K // 4):
            acc = T.mfma(Wb[n, 4 * j + g], yv[j], acc)
        for i in range(4):
            row = 16 * b + 4 * i + g
            live = row < K
            np.testing.assert_allclose(acc[live, i], Py[n[live], row[live]], rtol=1e-13, atol=1e-13)
            if 4 * b + i < K // 4:
                assert np.array_equal(row[live], (4 * (4 * b + i) + g)[live])
                quad = quad + np.where(live, yv[4 * b + i] * acc[:, i], 0.0)
    total = quad.reshape(4, 16).sum(axis=0)          # the four lane groups of a sample meet
    np.testing.assert_allclose(total, np.einsum("sr,sr->s", Y, Py), rtol=1e-12, atol=1e-12)


def test_envelope_by_formula():
    """Of the RESTATEMENT (which the GPU tests hold the library's answers to)."""
    a = S.corridor_set()
    small = T.smallest_window(a)
    assert T.served_by_formula(a) and T.served_by_formula(a, small) and not T.served_by_formula(a, small - 16)
    assert not T.served_by_formula(sweep.k65_case().arrays)
    for rows in T.CONES:          # a cone of any number of rows that fits a window is served, on both sides of one block
        assert T.served_by_formula(T.boundary_case(f"cone{rows}").arrays)
    c3 = cost_cases.case("c3").arrays
    assert T.width(c3["k"]) == 64 and len(T.partition(T.items(c3), 64, T.DEFAULT_WINDOW)) > 1
    for name in ("corridor_k12", "c5_shape", "past_limit64"):
        a = S.beyond_case(name).arrays
        assert len(T.partition(T.items(a), T.width(a["k"]), T.DEFAULT_WINDOW)) > 1, name
    k8 = T.k8_case().arrays
    assert [nw % 2 for _, nw in T.parity_windows(k8)] == [1, 0]


def test_binding_and_header_declare_the_same_entry_points():
    text = open(os.path.join(REPO, "include", "rayen_hip_cost_tile64.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.EXPORTS_COST_TILE64) and len(declared) == 3
    others = (_lib.EXPORTS, _lib.EXPORTS_TILE, _lib.EXPORTS_TILE64, _lib.EXPORTS_DC3_TILE, _lib.EXPORTS_DC3_TILE64,
              _lib.EXPORTS_COST_STREAM, _lib.EXPORTS_BAR_STREAM, _lib.EXPORTS_WIDE_FUSED, _lib.EXPORTS_WIDE_FUSED_BWD,
              _lib.EXPORTS_WIDE_FUSED64, _lib.EXPORTS_WIDE_FUSED_BWD64)
    assert not any(set(declared) & set(o) for o in others)
    assert '#include "rayen_hip_cost_tile64.h"' in open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    # argument checks that need no device
    assert lib.rayen_cost_tile64_set(None, 0) == -1 and lib.rayen_cost_tile64_served(None) == 0
    assert lib.rayen_soft_cost_tile64_f64(None, None, 0, 1, None, None, None, None, 0, None) == -1


def test_host_tensors_take_the_mirror_under_tile64():
    c = cost_cases.case("k17_m33")
    y = torch.from_numpy(c.y.copy())
    outs = []
    for sc in (SoftCost(c.cs), SoftCost(c.cs, kernel="tile64")):
        yy = y.clone().requires_grad_(True)
        cost = sc(yy)
        cost.sum().backward()
        outs.append((cost.detach(), yy.grad, *sc.violation(yy)))
    assert all(torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) for a, b in zip(*outs))
    y3 = y.float().unsqueeze(2)
    assert torch.equal(CostComputer(c.cs, fused=True, kernel="tile64").getSumSoftCostAllSamples(y3),
                       CostComputer(c.cs, fused=True).getSumSoftCostAllSamples(y3))


def test_keyword_validation():
    c = cost_cases.case("box3")
    assert "tile64" in KERNELS and "tile64" in ops.COST_KERNELS and "auto" not in ops.COST_KERNELS
    assert SoftCost(c.cs, kernel="tile64").kernel == "tile64"
    for bad in ("tile", "tile32", "Tile64", "", None):
        with pytest.raises(ValueError):
            SoftCost(c.cs, kernel=bad)
        with pytest.raises(ValueError):
            CostComputer(c.cs, fused=True, kernel=bad)
    with pytest.raises(ValueError):
        CostComputer(c.cs, kernel="tile64")          # (a route of the fused soft cost only)
    with pytest.raises(ValueError):
        ops.soft_cost_raw(torch.zeros(1, 3, dtype=torch.float64), None, False, kernel="tile32")
