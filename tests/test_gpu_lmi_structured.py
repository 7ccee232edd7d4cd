"""The LMI kernels on matrices with STRUCTURE (tests/lmi_structured_cases.py; proven well-posed by
tests/test_lmi_structured_host.py): the four-lane kernel (rayen_lmi_quad.h), the lane-per-sample kernel
(rayen_generic.hip), the wave-per-sample kernel (rayen_lmi_wave.h), the workgroup-per-sample kernel (rayen_lmi_block.h) and
the soft cost's (rayen_cost_lmi.hip) against the fp64 oracle, at the bars of tests/test_gpu_lmi_wave.py.  Zero Householder
columns, decoupled blocks, tied and nearly tied top eigenvalues, entries far from 1: no dense uniform generator reaches
these branches.  Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cost_lmi_cases                                         # noqa: E402
import lmi_structured_cases as S                              # noqa: E402
from helpers import rel_err_rows                              # noqa: E402
from rayen_amd import _lib, ops                               # noqa: E402
from rayen_amd.constraint_module import ConstraintModule      # noqa: E402

pytestmark = pytest.mark.gpu


def _kernel_of(name, family):
    if family == "quad" and S.case(name).r == 1:              # (the four-lane kernel starts at 2 x 2: module comment of TABLE)
        return _lib.KERNEL_LANE
    return {"quad": _lib.KERNEL_LMI_QUAD, "lane": _lib.KERNEL_LANE, "wave": _lib.KERNEL_LMI_WAVE,
            "block": _lib.KERNEL_LMI_BLOCK}[family]


def _pin(family, monkeypatch):
    """The environment of a kernel family; returns ``force_generic``."""
    if family in ("wave", "block"):
        monkeypatch.setenv("RAYEN_LMI_BLOCK", "1" if family == "block" else "0")
    else:
        monkeypatch.delenv("RAYEN_LMI_BLOCK", raising=False)
    return family == "lane"


@functools.lru_cache(maxsize=None)
def _device(name, dtype_name, polytope=False):
    """``(cs, layer, device pack)`` built under the matching default dtype (tests/test_gpu_lmi_wave.py::_layer)."""
    dtype = getattr(torch, dtype_name)
    raw = S.case(name).raw
    cs = S.build(S.polytope_raw(raw) if polytope else raw, dtype)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        layer = ConstraintModule(cs, create_map=False).cuda()
    finally:
        torch.set_default_dtype(prev)
    return cs, layer, layer.device_pack(torch.device("cuda", 0))[0]


def _bar(name, dtype_name):
    """fp64: 1e-9; fp32: 1e-5 or twice what LAPACK's fp32 eigvalsh leaves against the fp64 truth."""
    if dtype_name == "float64":
        return S.BAR["float64"]
    return max(S.BAR["float32"], 2.0 * float(S.lapack32_error(name).max()))


def _project(name, family, dtype_name, monkeypatch):
    generic = _pin(family, monkeypatch)
    _, _, dp = _device(name, dtype_name)
    xd = torch.from_numpy(S.case(name).x.copy()).to(getattr(torch, dtype_name)).cuda()
    y, kappa, active = ops.project_raw(xd, dp, want_active=True, force_generic=generic)
    fam = _lib.load().rayen_last_forward_kernel()
    assert fam == _kernel_of(name, family), (name, family, dtype_name, fam)
    return xd, y, kappa, active, dp, generic


@pytest.mark.parametrize("name,family,dtype_name", S.TRIPLES)
def test_forward_against_the_fp64_oracle(name, family, dtype_name, monkeypatch):
    c = S.case(name)
    cs64, ev = S.truth(name)
    _, y, kappa, _, _, _ = _project(name, family, dtype_name, monkeypatch)
    y = y.cpu().double().numpy()
    kap = kappa.cpu().double().numpy()
    err = rel_err_rows(y, ev["y"])
    bar = _bar(name, dtype_name)
    # kappa itself, against the size of S(v), at the same bar (a backward-stable eigen-solver is off by a small multiple of
    # r eps ||S||): the rows inside the set, where y = v whatever kappa is, are held to the oracle as well
    radius = np.abs(S.spectrum(c.raw, c.x)).max(axis=1)
    kerr = np.abs(kap - ev["kappa"]) / np.maximum(radius, 1e-300)
    kerr[2] = 0.0
    print(f"{name} {family} {dtype_name}: y {err.max():.3e} kappa {kerr.max():.3e} bar {bar:.1e}")
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(kap)) and np.all(kap >= 0)
    assert err.max() <= bar, (name, family, err.max(), int(np.argmax(err)))
    assert kerr.max() <= bar, (name, family, kerr.max(), int(np.argmax(kerr)))
    assert np.allclose(y[2], cs64.y0[:, 0], atol=1e-12 if dtype_name == "float64" else 1e-6)
    assert cs64.getMaxViolation(y) <= (1e-9 if dtype_name == "float64" else 2e-4)


@pytest.mark.parametrize("name,family,dtype_name", [t for t in S.TRIPLES if S.structure(t[0]) == "diag"])
def test_diagonal_lmi_against_the_same_set_as_linear_rows_on_the_device(name, family, dtype_name, monkeypatch):
    _, ev = S.truth(name)
    xd, y, _, _, _, _ = _project(name, family, dtype_name, monkeypatch)
    _, _, dp_lin = _device(name, dtype_name, polytope=True)
    y_lin = ops.project_raw(xd, dp_lin)[0].cpu().double().numpy()
    bar = _bar(name, dtype_name)
    assert rel_err_rows(y_lin, ev["y"]).max() <= bar
    assert rel_err_rows(y.cpu().double().numpy(), y_lin).max() <= bar


@pytest.mark.parametrize("name,family,dtype_name", [t for t in S.TRIPLES if S.structure(t[0]) in ("identity", "toeplitz")])
def test_intervals_in_closed_form_on_the_device(name, family, dtype_name, monkeypatch):
    c = S.case(name)
    _, y, _, _, _, _ = _project(name, family, dtype_name, monkeypatch)
    bound = -1.0 if c.structure == "identity" else S.toeplitz_bound(c.r)
    assert rel_err_rows(y.cpu().double().numpy(), np.maximum(c.x, bound)).max() <= _bar(name, dtype_name)


def _grad_y(c, dtype_name):
    gen = torch.Generator().manual_seed(6)
    return torch.empty(c.B, c.k).uniform_(-1, 1, generator=gen)


@functools.lru_cache(maxsize=None)
def _autograd(name):
    """grad_v of ``sum(y * g)`` through the fp64 oracle's eigvalsh, once per case."""
    c = S.case(name)
    cs64, _ = S.truth(name)
    ev = S.evaluate(cs64, c.x, grad=True)
    (ev["yt"][:, :, 0] * _grad_y(c, "float64").double()).sum().backward()
    want = ev["xt"].grad[:, :, 0].numpy().copy()
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("name,family,dtype_name", S.BACKWARD_SEPARATED)
def test_backward_on_separated_spectra(name, family, dtype_name, monkeypatch):
    """The bounds and the kink rule of tests/test_gpu_lmi_wave.py::_check_backward.  On blockdiag the eigenvector lives in
    one block and comes back through reflectors with tau = 0, on diag it is a unit vector."""
    c = S.case(name)
    _, ev = S.truth(name)
    dtype = getattr(torch, dtype_name)
    xd, _, kappa, active, dp, generic = _project(name, family, dtype_name, monkeypatch)
    g = _grad_y(c, dtype_name)
    got = ops.backward_raw(xd, kappa, active, g.to(dtype).cuda(), dp, force_generic=generic).cpu().double().numpy()
    want = _autograd(name)
    assert np.all(np.isfinite(got))
    size = np.maximum(np.abs(want).max(axis=1), 1e-30)
    gerr = np.abs(got - want).max(axis=1) / size
    gerr[2] = 0.0                                             # v = 0: eigvalsh of the zero matrix has no derivative worth comparing
    kink = S.kinks(ev["terms"], kappa.cpu().double().numpy(), dtype_name)
    tol = 2e-3 if dtype_name == "float32" else 1e-7
    eps = 6e-8 if dtype_name == "float32" else 1.1e-16
    bound = np.maximum(tol, 8.0 * c.r * eps / np.maximum(S.lam_gap(ev["terms"]), 1e-30))
    bad = (~kink) & ~(gerr <= bound)
    print(f"{name} {family} {dtype_name}: grad {np.max(np.where(kink, 0.0, gerr / bound)):.3f} of its bound, {int(kink.sum())} kinks")
    assert not bad.any(), (name, int(bad.sum()), np.flatnonzero(bad)[:5], gerr[bad][:5], bound[bad][:5])
    assert kink.sum() <= max(3, 0.05 * c.B)


@pytest.mark.parametrize("name,family,dtype_name", S.BACKWARD_TIED)
def test_backward_on_tied_spectra(name, family, dtype_name, monkeypatch):
    """The derivative is not unique where the top eigenvalues tie: the gradient is finite, rows inside the set pass
    ``g NA_E`` through (NA_E = I) and no row depends on another."""
    c = S.case(name)
    _, ev = S.truth(name)
    dtype = getattr(torch, dtype_name)
    xd, _, kappa, active, dp, generic = _project(name, family, dtype_name, monkeypatch)
    g = _grad_y(c, dtype_name).to(dtype).cuda()
    got = ops.backward_raw(xd, kappa, active, g, dp, force_generic=generic)
    assert bool(torch.isfinite(got).all())
    inside = torch.from_numpy((ev["kappa"] < 0.999) & (kappa.cpu().double().numpy() < 1.0)).cuda()
    assert int(inside.sum()) >= 2
    assert float((got - g)[inside].abs().max()) <= (1e-5 if dtype_name == "float32" else 1e-12)
    part = ops.backward_raw(xd[:7].contiguous(), kappa[:7].contiguous(), active[:7].contiguous(), g[:7].contiguous(), dp,
                            force_generic=generic)
    assert torch.equal(part, got[:7])


AGREE = [("diag_r5", "quad", "lane"), ("blockdiag_3_2", "quad", "lane"), ("twin_r5_{t}", "quad", "lane"),
         ("zero_line_r16_j8", "quad", "lane"), ("twin_r16_{t}_rev", "quad", "lane"), ("graded{p}_r16", "quad", "lane")]
AGREE_BIG = [("blockdiag_19_14", "float32"), ("twin_r33_1e-4", "float32"), ("zero_line_r33_j0", "float32"),
             ("blockdiag_25_19", "float64"), ("twin_r44_7e-9", "float64"), ("zero_line_r44_j43", "float64")]


@pytest.mark.parametrize("name,dtype_name,first,second",
                         [(n.format(t="1e-4" if d == "float32" else "7e-9", p=3 if d == "float32" else 6), d, a, b)
                          for n, a, b in AGREE for d in ("float32", "float64")]
                         + [(n, d, "wave", "block") for n, d in AGREE_BIG])
def test_two_families_on_one_size_both_meet_the_oracle_bar(name, dtype_name, first, second, monkeypatch):
    """quad and lane at r = 5 and 16, wave and block at r = 33 (fp32) and r = 44 (fp64): the same answers to the bar, not
    bit for bit (different reflectors, different bisections)."""
    _, ev = S.truth(name)
    bar = _bar(name, dtype_name)
    ys = []
    for family in (first, second):
        _, y, _, _, _, _ = _project(name, family, dtype_name, monkeypatch)
        ys.append(y.cpu().double().numpy())
        assert rel_err_rows(ys[-1], ev["y"]).max() <= bar, (name, family)
    assert rel_err_rows(ys[0], ys[1]).max() <= 2.0 * bar


@pytest.mark.parametrize("name,dtype_name", S.COST_TRIPLES)
def test_soft_cost_on_structured_sets(name, dtype_name):
    """rayen_cost_lmi.hip tridiagonalises with the wave kernel's routine and takes lambda_min(F(y)): values and gradient on
    the plain rows, against tests/cost_lmi_cases.py's reference at its bars."""
    c = S.cost_case(name)
    pack = ops.CostPack(c.arrays, torch.cuda.current_device())
    assert pack.served(getattr(torch, dtype_name))
    y = torch.from_numpy(c.y.copy()).to(getattr(torch, dtype_name)).cuda()
    out = ops.soft_cost_raw(y, pack, True)
    cost_lmi_cases.check(c, dtype_name, *(t.detach().cpu().numpy() for t in out), f"{name} {dtype_name} structured")
    assert c.finite.all() and (c.ref["lmi"]["g"] > 0).sum() >= c.B / 4
