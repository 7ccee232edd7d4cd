"""The wide kernels (n > 128: rayen_wide_fused.hip, rayen_wide_fused_bwd.hip, rayen_wide.hip) on an MI355X, swept: crafted
block plans on real geometry against fp64 on the same pack (tests/wide_sweep_cases.py; tests/test_wide_sweep_host.py holds the
plans to what their names promise), and second rounds of every persistent and grid-stride loop, bit for bit against the
300 rows the older files hold to fp64.

Bars: kappa within 1e-5 max(1, kappa64); y within ``FP32_TOL`` by ``rel_err_rows``; ``active`` a maximiser in fp64 by the
rule of tests/test_gpu_wide_fused.py; grad_v within ``GRAD_TOL[float32]`` by ``_row_err`` on non-kink rows
(``wide_sweep_cases.kink_rows``).  The packs are created without the inward bias: the truth is fp64 on the very rows."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_fused_bwd_cases as WB                             # noqa: E402
import wide_fused_cases as F                                  # noqa: E402
import wide_sweep_cases as S                                  # noqa: E402
from helpers import rel_err_rows                              # noqa: E402
from rayen_amd import _lib, ops                               # noqa: E402
from rayen_amd.constraint_module import ConstraintModule      # noqa: E402
from rayen_amd.pack import DevicePack                         # noqa: E402
from test_gpu_backward import GRAD_TOL, _row_err              # noqa: E402
from test_gpu_parity import FP32_TOL                          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LIN = _lib.SEG_LIN
ROUTES = ("fused", "products")
KERNEL = {"fused": _lib.KERNEL_WIDE_FUSED, "products": _lib.KERNEL_PRODUCTS}
_PACKS, _RECORDS = {}, {}


def _pack(key):
    """The device pack of a case (``name``), of its packer layout (``name + ':packed'``), of ``gaps`` with the rows of
    nobody zero (``'gaps:zero'``) or of a set of the two older files (``'old:' + name``); built once."""
    if key not in _PACKS:
        if key.startswith("old:"):
            consts = ConstraintModule(WB.cs(key[4:]), create_map=False).packed_constants()
        elif key.endswith(":packed"):
            consts = S.packed(key[:-7])
        elif key == "gaps:zero":
            consts = S.zero_gaps(S.consts("gaps"))
        else:
            consts = S.consts(key)
        _PACKS[key] = DevicePack(consts, 0)
    return _PACKS[key]


def _forward(key, v, route, **kw):
    dp = _pack(key)
    out = ops.project_raw(v, dp, wide_kernel=route, **kw)
    assert _lib.load().rayen_last_forward_kernel() == KERNEL[route]
    assert int(dp.nan_flag.item()) == 0
    return out


def _records(name):
    """(v, kappa, active, G) of a case on the device, from the products forward; once per case."""
    if name not in _RECORDS:
        v = S.inputs(name)[:, :, 0].cuda()
        _, kappa, active = _forward(name, v, "products")
        _RECORDS[name] = (v, kappa, active, S.grads(name).cuda())
    return _RECORDS[name]


def _backward(key, v, kappa, active, G, how):
    """``how``: 'products' | 'fused' (grouped) | 'fused_batch_order'."""
    if how == "products":
        return ops.backward_raw(v, kappa, active, G, _pack(key))
    return ops.backward_raw(v, kappa, active, G, _pack(key), wide_backward="fused", group=how == "fused")


BACKWARDS = ("products", "fused", "fused_batch_order")


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ B. the crafted plans
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", S.CASES)
def test_forward_against_fp64_on_the_relaid_pack(name, route):
    y64, k64, _, _ = S.truth(name)
    v = S.inputs(name)[:, :, 0].cuda()
    y, kappa, active = _forward(name, v, route)
    scale = np.maximum(1.0, k64)
    err_k = np.abs(kappa.double().cpu().numpy() - k64) / scale
    err_y = rel_err_rows(y.cpu().numpy(), y64)
    print(f"SWEEP forward {name} {route}: kappa error / bar {err_k.max() / 1e-5:.3f}, y error / bar {err_y.max() / FP32_TOL:.3f}")
    assert np.all(err_k <= 1e-5)
    assert np.max(err_y) <= FP32_TOL
    consts = S.consts(name)
    WB.assert_active_names_a_maximiser(consts, v.double().cpu().numpy(), k64, active.cpu().numpy())
    assert np.array_equal(y[8].cpu().numpy(), consts.y0.astype(np.float32))          # the zero direction returns y0


@pytest.mark.parametrize("name", S.CASES)
def test_backward_against_fp64_autograd_on_the_relaid_pack(name):
    want = S.truth(name)[3]
    v, kappa, active, G = _records(name)
    kink = S.kink_rows(name, v.double().cpu().numpy())
    assert kink.sum() <= 3
    got = {}
    for how in BACKWARDS:
        got[how] = _backward(name, v, kappa, active, G, how)
        g = got[how].double().cpu().numpy()
        assert np.all(np.isfinite(g)), how
        err = _row_err(g, want)
        print(f"SWEEP backward {name} {how}: worst row error / bar {err[~kink].max() / GRAD_TOL[torch.float32]:.3f} "
              f"(kink rows {int(kink.sum())})")
        bad = ~kink & ~(err <= GRAD_TOL[torch.float32])
        assert not bad.any(), (how, np.flatnonzero(bad)[:5], err[bad][:5])
    # the fused kernel: the same bits grouped or in batch order, and on the batch flipped
    assert torch.equal(got["fused"], got["fused_batch_order"])
    flipped = [t.flip(0).contiguous() for t in (v, kappa, active, G)]
    for how in ("fused", "fused_batch_order"):
        assert torch.equal(_backward(name, *flipped, how).flip(0), got["fused"]), how


def _pairs(consts):
    seen, out = {}, []
    for si, s in enumerate(consts.segments):
        if s.type != LIN:
            continue
        for r in range(s.row0, s.row0 + s.nrows):
            key = consts.W[r].tobytes()
            if key in seen:
                out.append((seen[key], (si, r)))
            else:
                seen[key] = (si, r)
    return out


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["lin_ties", "lin_ties_cut"])
def test_an_exact_tie_goes_to_the_lower_row_and_the_earlier_segment(name, route):
    consts = S.consts(name)
    v = S.inputs(name)[:, :, 0].cuda()
    _, kappa, active = _forward(name, v, route)
    active = active.cpu().numpy()
    v64 = v.double().cpu().numpy()
    k64 = S.truth(name)[1]
    T = v64 @ consts.W.T
    kink = S.kink_rows(name, v64)
    pairs = _pairs(consts)
    assert len(pairs) == 3
    for (seg_lo, lo), (seg_hi, hi) in pairs:
        assert lo < hi and seg_lo <= seg_hi
        rows = np.flatnonzero((k64 > 0) & (T[:, lo] == k64) & ~kink)          # the copied row is THE maximiser in fp64
        assert len(rows) >= 5, (lo, hi)
        assert np.all(active[rows, 0] == seg_lo) and np.all(active[rows, 1] == lo), (lo, hi, active[rows])
    if name == "lin_ties_cut":
        assert any(seg_lo < seg_hi for (seg_lo, _), (seg_hi, _) in pairs)
    # kappa: the bits of the pack without the copies wherever a linear row sets it (a row's product does not depend on
    # where the row sits).  The fused kernel promises that; the products route goes through a library GEMM whose shape
    # changes with the row count: its count is a report.
    _, plain, plain_active = _forward("lin_ties_plain", v, route)
    by_lin = torch.as_tensor([s.type == LIN for s in S.consts("lin_ties_plain").segments] + [False], device=DEV)
    on_lin = by_lin[plain_active[:, 0].long()]
    assert int(on_lin.sum()) >= 60
    same = kappa[on_lin] == plain[on_lin]
    print(f"SWEEP lin_ties {name} {route}: kappa bits equal on {int(same.sum())} of {int(on_lin.sum())} rows a linear row sets")
    if route == "fused":
        assert bool(same.all())


@pytest.mark.parametrize("name", list(S.NBW))
def test_a_linear_rows_product_does_not_depend_on_where_the_row_sits(name):
    v = S.inputs(name)[:, :, 0].cuda()
    for route in ROUTES:
        _, kappa, active = _forward(name, v, route)
        _, kappa_p, active_p = _forward(name + ":packed", v, route)
        lin = [i for i, s in enumerate(S.consts(name).segments) if s.type == LIN]
        lin_p = [i for i, s in enumerate(S.packed(name).segments) if s.type == LIN]
        assert lin == lin_p == [0]
        on_lin = (active[:, 0] == 0) & (active_p[:, 0] == 0)
        assert int(on_lin.sum()) >= 40
        same = kappa[on_lin] == kappa_p[on_lin]
        print(f"SWEEP row position {name} {route}: kappa bits equal on {int(same.sum())} of {int(on_lin.sum())} rows")
        # (the products route too: the two packs have the same row count, so the library GEMM is the same one)
        assert bool(same.all()), route
        row0, row0_p = S.consts(name).segments[0].row0, S.packed(name).segments[0].row0
        assert torch.equal(active[on_lin, 1] - row0, active_p[on_lin, 1] - row0_p), route


def test_rows_of_no_segment_change_no_bit():
    v, kappa, active, G = _records("gaps")
    for route in ROUTES:
        assert _same(_forward("gaps", v, route), _forward("gaps:zero", v, route)), route
    for how in BACKWARDS:
        assert torch.equal(_backward("gaps", v, kappa, active, G, how), _backward("gaps:zero", v, kappa, active, G, how)), how


@pytest.mark.parametrize("name", ["eq_k191", "soc_straddle"])
def test_output_buffer_variants(name):
    consts = S.consts(name)
    n, k = consts.n, consts.k
    assert bool(consts.out_identity) == (name == "soc_straddle")
    v, kappa0, active0, G = _records(name)
    wide_v = torch.full((S.B, n + 7), float("nan"), device=DEV)
    wide_v[:, :n] = v
    for route in ROUTES:
        y, kappa, active = _forward(name, v, route)
        yn, kn, an = _forward(name, v, route, want_y=False)
        assert yn is None and torch.equal(kn, kappa) and torch.equal(an, active), route
        buf = torch.full((S.B, k + 5), -7.0, device=DEV)
        yo, ko, ao = _forward(name, v, route, out=buf)
        assert yo is buf and torch.equal(buf[:, :k], y) and bool((buf[:, k:] == -7.0).all()), route
        assert torch.equal(ko, kappa) and torch.equal(ao, active), route
        assert _same(_forward(name, wide_v[:, :n], route), (y, kappa, active)), route          # ldv > n, the rest unread
    for how in BACKWARDS:
        full = _backward(name, v, kappa0, active0, G, how)
        assert torch.equal(_backward(name, wide_v[:, :n], kappa0, active0, G, how), full), how
        padded = wide_v.clone()
        padded[:, n:] = 3.0
        got = _backward(name, padded, kappa0, active0, G, how)          # v wider than n: the extra columns of grad_v are zero
        assert got.shape == (S.B, n + 7) and torch.equal(got[:, :n], full) and bool((got[:, n:] == 0).all()), how


# ------------------------------------------------------------------------------------------------ C. second rounds
RESERVE = 128           # the largest value rayen_reserve_cus accepts: the grids at their smallest


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class _reserved:
    def __init__(self, cus):
        self.cus = cus

    def __enter__(self):
        self.prev = _lib.load().rayen_reserve_cus(self.cus)

    def __exit__(self, *exc):
        _lib.load().rayen_reserve_cus(self.prev)


def _old_plans(name):
    return S.plans(_pack("old:" + name).consts)


_BASE = {}


def _base(name):
    """The 300 rows of a set of the older files and their outputs at no reservation: (v, G, (y, kappa, active) of the fused
    forward, grad_v of the fused backward on those records)."""
    if name not in _BASE:
        assert _lib.load().rayen_reserve_cus(-1) == 0
        v, G = WB.inputs(name)[:, :, 0].cuda(), WB.grads(name).cuda()
        fwd = _forward("old:" + name, v, "fused")
        _BASE[name] = (v, G, fwd, _backward("old:" + name, v, fwd[1], fwd[2], G, "fused"))
    return _BASE[name]


def _idx(B, seed=5):
    """A fixed map of B rows onto the 300: every tile mixes rows of several active segments."""
    return torch.randint(0, 300, (B,), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _three_rounds(slots):
    B = S.second_round_batch(slots)
    n_tiles = -(-B // 32)
    assert n_tiles > 2 * F.grid(B, slots) and B % 32 != 0          # every workgroup a second round, most a third
    return B


@pytest.mark.parametrize("name", ["mixI", "mixE", "k1024"])
def test_fused_forward_second_and_third_rounds(name):
    lib = _lib.load()
    assert lib.rayen_reserve_cus(-1) == 0
    v300, _, (y300, k300, a300), _ = _base(name)
    fp, _, _ = _old_plans(name)
    slots = F.slots_fwd(fp, F.launch_cus(_cus(), RESERVE))
    assert (slots // F.launch_cus(_cus(), RESERVE) == 1) == (name == "k1024")          # a 128 KiB tile: one workgroup a CU
    B = _three_rounds(slots)
    idx = _idx(B)
    v = v300[idx]
    with _reserved(RESERVE):
        y, kappa, active = _forward("old:" + name, v, "fused")
        yn, kn, an = _forward("old:" + name, v, "fused", want_y=False)
    assert torch.equal(kappa, k300[idx]) and torch.equal(active, a300[idx]) and torch.equal(y, y300[idx])
    assert yn is None and torch.equal(kn, kappa) and torch.equal(an, active)
    assert lib.rayen_reserve_cus(-1) == 0


@pytest.mark.parametrize("name", ["mixI", "mixE"])
def test_fused_backward_second_and_third_rounds(name):
    lib = _lib.load()
    assert lib.rayen_reserve_cus(-1) == 0
    v300, G300, (_, k300, a300), g300 = _base(name)
    _, _, bp = _old_plans(name)
    B = _three_rounds(WB.slots_bwd(bp, F.launch_cus(_cus(), RESERVE)))
    idx = _idx(B, seed=6)
    args = (v300[idx], k300[idx], a300[idx], G300[idx])
    with _reserved(RESERVE):
        for how in ("fused", "fused_batch_order"):
            assert torch.equal(_backward("old:" + name, *args, how), g300[idx]), how
    assert lib.rayen_reserve_cus(-1) == 0


def test_grouping_kernels_second_and_third_rounds():
    """The count and scatter kernels stride beyond 256 rows a SIMD: two whole rounds and a partial third."""
    lib = _lib.load()
    assert lib.rayen_reserve_cus(-1) == 0
    v300, G300, (_, k300, a300), g300 = _base("mixI")
    half = F.launch_cus(_cus(), RESERVE)
    B = 2 * 256 * 4 * half + 256 + 77
    assert -(-B // 256) > 2 * WB.grouping_grid(B, half) and B % 256 != 0
    assert lib.rayen_wide_fused_bwd_workspace_bytes(_pack("old:mixI").handle, B) > 0
    idx = _idx(B, seed=7)
    v, kappa, active, G = v300[idx], k300[idx], a300[idx], G300[idx]
    with _reserved(RESERVE):
        got = _backward("old:mixI", v, kappa, active, G, "fused")
    want = g300[idx]
    same = torch.equal(got, want)
    del v, kappa, active, G, got, want, idx
    torch.cuda.empty_cache()
    assert same
    assert lib.rayen_reserve_cus(-1) == 0


@pytest.mark.parametrize("name", ["mixI", "mixE"])
def test_products_route_strides_its_grid(name):
    """``wide_epilogue_kernel`` and ``wide_bwd_coeff_kernel`` stride beyond four rows a workgroup, two workgroups a SIMD.  The
    library GEMM may change with B: against the fp64 kernels on the same rows, under the bars above."""
    lib = _lib.load()
    assert lib.rayen_reserve_cus(-1) == 0
    v300, G300, _, _ = _base(name)
    half = F.launch_cus(_cus(), RESERVE)
    B = 4 * 2 * 4 * half * 2 + 4 * 2 * 4 * half // 2 + 13          # two rounds and a half of the capped grid
    assert -(-B // 4) > 2 * (2 * 4 * half)
    idx = _idx(B, seed=8)
    v, G = v300[idx], G300[idx]
    dp = _pack("old:" + name)
    kink300 = S.kink_rows(dp.consts, v300.double().cpu().numpy())
    kink = kink300[idx.cpu().numpy()]
    with _reserved(RESERVE):
        y, kappa, active = _forward("old:" + name, v, "products")
        grad = _backward("old:" + name, v, kappa, active, G, "products")
        y64, k64, a64 = ops.project_raw(v.double(), dp)
        g64 = ops.backward_raw(v.double(), k64, a64, G.double(), dp)
    assert lib.rayen_reserve_cus(-1) == 0
    k64n = k64.cpu().numpy()
    err_k = np.abs(kappa.double().cpu().numpy() - k64n) / np.maximum(1.0, k64n)
    err_y = rel_err_rows(y.cpu().numpy(), y64.cpu().numpy())
    err_g = _row_err(grad.double().cpu().numpy(), g64.cpu().numpy())
    print(f"SWEEP products {name} B = {B}: kappa error / bar {err_k.max() / 1e-5:.3f}, y error / bar {err_y.max() / FP32_TOL:.3f}, "
          f"gradient error / bar {err_g[~kink].max() / GRAD_TOL[torch.float32]:.3f} (kink rows among the 300: "
          f"{int(kink300.sum())})")
    assert np.all(err_k <= 1e-5) and np.max(err_y) <= FP32_TOL
    assert np.all(err_g[~kink] <= GRAD_TOL[torch.float32])


@pytest.mark.parametrize("name", ["mixI", "mixE"])
def test_reserved_compute_units_change_the_launch_not_the_bits(name):
    lib = _lib.load()
    assert lib.rayen_reserve_cus(-1) == 0
    v300, G300, fwd300, g300 = _base(name)
    fp, _, bp = _old_plans(name)
    B = _three_rounds(F.slots_fwd(fp, F.launch_cus(_cus(), RESERVE)))
    idx = _idx(B, seed=9)
    big = (v300[idx], G300[idx], tuple(t[idx] for t in fwd300), g300[idx])
    for v, G, fwd, grad in ((v300, G300, fwd300, g300), big):
        for cus in (0, 8, RESERVE):
            with _reserved(cus):
                assert _same(_forward("old:" + name, v, "fused"), fwd), (cus, v.shape[0])
                for how in ("fused", "fused_batch_order"):
                    assert torch.equal(_backward("old:" + name, v, fwd[1], fwd[2], G, how), grad), (cus, how, v.shape[0])
    assert lib.rayen_reserve_cus(-1) == 0
