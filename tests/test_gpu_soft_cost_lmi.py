"""Soft cost and violation of sets with an LMI on the kernel of rayen_amd/csrc/rayen_cost_lmi.hip: through
``rayen_amd::soft_cost``, ``ops.soft_cost_raw``, the raw C ABI and ``SoftCost``, against the fp64 reference and at the bars
of tests/cost_lmi_cases.py (its docstring derives them; tests/test_cost_lmi_reference_host.py shows that they reject wrong
answers).  Every test that goes through ``ops.CostPack`` fails without ``rayen_cost_pack_set_lmi``.  Needs an MI355X."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cost_cases                                             # noqa: E402
import cost_lmi_cases as L                                    # noqa: E402
import cost_reference                                         # noqa: E402
from helpers import cost_check, cost_device_y                 # noqa: E402
from rayen_amd import _lib, ops, soft_cost                    # noqa: E402
from rayen_amd.cost_computer import CostComputer              # noqa: E402
from rayen_amd.soft_cost import SoftCost                      # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ["float32", "float64"]
ALL = [(n, B, d) for n in L.SERVED for B in L.BATCHES for d in DTYPES if L.served(n, d)]
LARGE = [(n, d) for n in L.SERVED for d in DTYPES if L.served(n, d)]
_PACKS = {}


def _pack(name, part="all"):
    """The device pack of a set (``all``), of its rows without the LMI (``rows``) or of its LMI alone (``lmi``)."""
    if (name, part) not in _PACKS:
        _, arrays, rows, alone = L.the_set(name)
        _PACKS[name, part] = ops.CostPack({"all": arrays, "rows": rows, "lmi": alone}[part], torch.cuda.current_device())
    return _PACKS[name, part]


def _y(c, dtype_name):
    return torch.from_numpy(c.y.copy()).to(getattr(torch, dtype_name)).cuda()


def _host(*tensors):
    return tuple(None if t is None else t.detach().cpu().numpy() for t in tensors)


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.mark.parametrize("name,B,dtype_name", ALL)
def test_raw_against_the_reference(name, B, dtype_name):
    c = L.case(name, B)
    pack = _pack(name)
    assert pack.served(getattr(torch, dtype_name))
    y = _y(c, dtype_name)
    cost, worst, which, grad = ops.soft_cost_raw(y, pack, True)
    ref = L.check(c, dtype_name, *_host(cost, worst, which, grad), f"{name} B={B} {dtype_name} raw")
    if name in L.MIXED and B == 67:                           # every index after the LMI is one higher than without it
        assert (ref["which"][c.finite] == ref["lmi_id"]).any()
        assert (ref["which"][c.finite] > ref["lmi_id"]).any() == (ref["n_eq"] > 0)
    # values alone (grad = NULL): the same cost, bit for bit; a second call repeats the first
    cost0, worst0, which0, none = ops.soft_cost_raw(y, pack, False)
    cost2, worst2, which2, grad2 = ops.soft_cost_raw(y, pack, True)
    assert none is None
    for a, b in ((cost0, cost), (worst0, worst), (cost2, cost), (worst2, worst), (grad2, grad)):
        assert _same(a, b)
    assert torch.equal(which0, which) and torch.equal(which2, which)
    # the NaN row's neighbours: bit-identical to a run without it
    bad = np.flatnonzero(~c.finite)
    if len(bad):
        clean = y.clone()
        clean[bad] = 0.0
        costc, worstc, whichc, gradc = ops.soft_cost_raw(clean, pack, True)
        keep = torch.from_numpy(c.finite).cuda()
        assert torch.equal(costc[keep], cost[keep]) and torch.equal(worstc[keep], worst[keep])
        assert torch.equal(whichc[keep], which[keep]) and torch.equal(gradc[keep], grad[keep])
        assert bool(torch.isfinite(costc).all())


@pytest.mark.parametrize("name,dtype_name", LARGE)
def test_op_and_module_against_the_reference(name, dtype_name):
    c = L.case(name, 67)
    pack = _pack(name)
    y = _y(c, dtype_name).requires_grad_(True)
    cost, worst, which, grad = torch.ops.rayen_amd.soft_cost(y, ops.register_pack(pack), True)
    L.check(c, dtype_name, *_host(cost, worst, which, grad), f"{name} {dtype_name} op")
    (gy,) = torch.autograd.grad(cost.sum(), y)
    assert _same(gy, grad)
    # the module: forward + autograd, violation; no mirror (strict mode would raise, a warning is an error here)
    sc = SoftCost(c.cs).cuda()
    ym = _y(c, dtype_name).unsqueeze(2).requires_grad_(True)
    loss = sc(ym)
    loss.sum().backward()
    mworst, mwhich = sc.violation(ym)
    assert sc._cost_packs and not sc._unsupported
    L.check(c, dtype_name, *_host(loss, mworst, mwhich, ym.grad[:, :, 0]), f"{name} {dtype_name} module")


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("name", L.MIXED)
def test_mixed_set_is_the_rows_launch_plus_the_lmi_alone(name, dtype_name):
    """The accumulating launch adds and never overwrites: the set's result is the existing kernel's on the set without its
    LMI combined on the host with the result of the LMI alone -- exactly (the kernel rounds its products before it adds)."""
    c = L.case(name, 67)
    y = _y(c, dtype_name)
    cost, worst, which, grad = ops.soft_cost_raw(y, _pack(name), True)
    rcost, rworst, rwhich, rgrad = ops.soft_cost_raw(y, _pack(name, "rows"), True)
    lcost, lworst, lwhich, lgrad = ops.soft_cost_raw(y, _pack(name, "lmi"), True)
    ok = torch.from_numpy(c.finite).cuda()
    lmi_id = c.ref["lmi_id"]
    assert bool((lwhich[ok] == 0).all()) and bool((lwhich[~ok] == -1).all())
    assert torch.equal(cost[ok], (rcost + lcost)[ok]) and torch.equal(grad[ok], (rgrad + lgrad)[ok])
    assert bool((lcost[ok] > 0).any()) and bool((rcost[ok] > 0).any()) and bool((lcost[ok] == 0).any())
    lmi_wins = (lworst > rworst) | ((lworst == rworst) & (rwhich >= lmi_id))
    want_worst = torch.where(lmi_wins, lworst, rworst)
    want_which = torch.where(lmi_wins, torch.full_like(rwhich, lmi_id), rwhich + (rwhich >= lmi_id).to(rwhich.dtype))
    assert torch.equal(worst[ok], want_worst[ok]) and torch.equal(which[ok], want_which[ok])
    assert bool(lmi_wins[ok].any()) and bool((~lmi_wins)[ok].any())
    if c.ref["n_eq"]:
        assert bool((which[ok] > lmi_id).any())               # an equality row on top, its index moved up by one
    assert bool(torch.isnan(cost[~ok]).all()) and bool(torch.isnan(worst[~ok]).all()) and bool((which[~ok] == -1).all())


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("name", ["k10_r20", "k70_r12", "lin5_eq2_lmi8"])
def test_raw_abi_strided_gradient_and_canaries(name, dtype_name):
    """Straight through ctypes: caller-owned buffers, a y and a gradient with row strides of their own (columns beyond k hold
    NaN / canaries: never read, never written), canaries around everything."""
    c = L.case(name, 67)
    lib, pack = _lib.load(), _pack(name)
    dtype = getattr(torch, dtype_name)
    B, k, ldg = c.B, c.k, c.k + 5
    wide = torch.full((B, k + 3), float("nan"), dtype=dtype, device="cuda")
    wide[:, :k] = _y(c, dtype_name)
    y = wide[:, :k]
    canary = 12345.0
    cost = torch.full((B + 2,), canary, dtype=dtype, device="cuda")
    worst = torch.full((B + 2,), canary, dtype=dtype, device="cuda")
    which = torch.full((B + 2,), 777, dtype=torch.int32, device="cuda")
    grad = torch.full((B + 2, ldg), canary, dtype=dtype, device="cuda")
    fn = lib.rayen_soft_cost_f32 if dtype_name == "float32" else lib.rayen_soft_cost_f64
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = fn(pack.handle, y.data_ptr(), B, y.stride(0), cost[1:].data_ptr(), worst[1:].data_ptr(), which[1:].data_ptr(),
              grad[1:].data_ptr(), ldg, stream)
    assert code == 0
    torch.cuda.synchronize()
    L.check(c, dtype_name, *_host(cost[1:B + 1], worst[1:B + 1], which[1:B + 1], grad[1:B + 1, :k]), f"{name} {dtype_name} abi")
    for t in (cost, worst, grad):
        assert float(t[0].flatten()[0]) == canary and float(t[B + 1].flatten()[0]) == canary
    assert int(which[0]) == 777 and int(which[B + 1]) == 777
    assert bool((grad[:, k:] == canary).all()) and bool((grad[0] == canary).all()) and bool((grad[B + 1] == canary).all())
    # the same rows from the dense call, bit for bit; argument checks; B = 0
    dcost, dworst, dwhich, dgrad = ops.soft_cost_raw(_y(c, dtype_name), pack, True)
    assert _same(dcost, cost[1:B + 1]) and _same(dworst, worst[1:B + 1]) and _same(dgrad, grad[1:B + 1, :k])
    assert torch.equal(dwhich, which[1:B + 1])
    assert fn(pack.handle, y.data_ptr(), B, k - 1, cost.data_ptr(), None, None, None, 0, None) == -1
    assert fn(pack.handle, None, 0, k, None, None, None, None, 0, None) == 0
    if name in L.MIXED:       # two launches: the second compares with the stored worst
        assert fn(pack.handle, y.data_ptr(), B, y.stride(0), None, None, which[1:].data_ptr(), None, 0, stream) == -1


def test_a_second_lmi_and_bad_sizes_are_refused():
    lib = _lib.load()
    _, arrays, _, _ = L.the_set("k4_r3")
    pack = ops.CostPack(arrays, torch.cuda.current_device())
    F = arrays["F"]
    assert lib.rayen_cost_pack_set_lmi(pack.handle, F.ctypes.data, 3) == -1          # RAYEN_E_BAD_ARG: it has one
    bare = ops.CostPack(dict(arrays, F=np.zeros((0, 0, 0))), torch.cuda.current_device())
    assert not bare.served(torch.float32) and not bare.served(torch.float64)        # no rows, no LMI yet
    assert lib.rayen_cost_pack_set_lmi(bare.handle, F.ctypes.data, 0) == -1
    assert lib.rayen_cost_pack_set_lmi(bare.handle, None, 3) == -1
    assert lib.rayen_cost_pack_set_lmi(None, F.ctypes.data, 3) == -1
    assert lib.rayen_cost_pack_set_lmi(bare.handle, F.ctypes.data, 3) == 0
    assert bare.served(torch.float32) and bare.served(torch.float64)
    assert lib.rayen_cost_pack_set_lmi(bare.handle, F.ctypes.data, 3) == -1
    c = L.case("k4_r3", 3)
    for a, b in zip(ops.soft_cost_raw(_y(c, "float64"), bare, True), ops.soft_cost_raw(_y(c, "float64"), pack, True)):
        assert _same(a, b)


@pytest.mark.eager_detour
@pytest.mark.parametrize("name,dtype_name", [("k5_over32", "float32"), ("k5_over32", "float64"), ("k5_over64", "float64")])
def test_over_limit_set_is_refused_and_the_module_runs_the_mirror(name, dtype_name, monkeypatch):
    """One r above the largest each precision serves.  (The suite's conftest keeps every other GPU test under
    RAYEN_STRICT_HIP=1; this one manages the variable itself.)"""
    cs, arrays, _, _ = L.the_set(name)
    dtype = getattr(torch, dtype_name)
    pack = ops.CostPack(arrays, torch.cuda.current_device())
    assert not pack.served(dtype) and pack.served(torch.float32) == L.served(name, "float32")
    k = L.SETS[name][0]
    y = torch.from_numpy(np.random.default_rng(3).uniform(-1.0, 1.0, size=(5, k))).to(dtype).cuda()
    with pytest.raises(_lib.RayenError) as err:
        ops.soft_cost_raw(y, pack, True)
    assert err.value.code == _lib.E_UNSUPPORTED
    monkeypatch.delenv("RAYEN_STRICT_HIP", raising=False)
    sc = SoftCost(cs).cuda()
    yg = y.clone().requires_grad_(True)
    with pytest.warns(RuntimeWarning, match="no HIP kernel serves"):
        cost = sc(yg)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cost_again = sc(yg)
        worst, which = sc.violation(yg)
    want_cost, want_worst, want_which = soft_cost.mirror(sc.constants(dtype, y.device), y)
    assert torch.equal(cost, cost_again) and torch.equal(cost.detach(), want_cost)
    assert torch.equal(worst, want_worst) and torch.equal(which, want_which)
    monkeypatch.setenv("RAYEN_STRICT_HIP", "1")
    with pytest.raises(_lib.RayenError):
        SoftCost(cs).cuda()(y)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_device_tensors_of_a_served_lmi_set_never_reach_the_mirror(dtype_name, monkeypatch):
    def no_mirror(*args, **kwargs):
        raise AssertionError("the torch mirror was called for a served set on a device tensor")
    monkeypatch.setattr(soft_cost, "mirror", no_mirror)
    c = L.case("k10_r20", 67)
    sc = SoftCost(c.cs).cuda()
    y = _y(c, dtype_name).requires_grad_(True)
    cost = sc(y)
    cost.sum().backward()
    worst, which = sc.violation(y)
    L.check(c, dtype_name, *_host(cost, worst, which, y.grad), f"k10_r20 {dtype_name} no mirror")


def test_fused_cost_computer_reaches_the_kernel():
    c = L.case("k10_r20", 67)
    ok = torch.from_numpy(c.finite).cuda()
    y = _y(c, "float32")[ok].unsqueeze(2).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        computer = CostComputer(c.cs, fused=True).cuda()
        loss = computer.getSumSoftCostAllSamples(y)
        loss.backward()
    assert computer.soft_cost._cost_packs and not computer.soft_cost._unsupported
    ref, d = L.value_bar(c, "float32")
    g = ref["lmi"]["g"][c.finite]
    bar = np.sum(2.0 * np.abs(g) * d[c.finite] + d[c.finite] ** 2)
    want = float(np.sum(ref["cost"][c.finite]))
    assert abs(loss.item() - want) <= bar + 67 * 2.0 ** -24 * want
    with pytest.raises(NotImplementedError):                  # unchanged
        computer.getInequalityValues(y.detach())


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_pack_without_an_lmi_answers_as_before(dtype_name):
    """The equality rows' offset is 0 without an LMI: their ``which`` is the unshifted index, the answers are those of the
    reference of tests/cost_reference.py and two runs agree bit for bit."""
    c = cost_cases.case("lin5_eq2")
    pack = ops.CostPack(c.arrays, torch.cuda.current_device())
    y = cost_device_y(c, dtype_name)
    first = ops.soft_cost_raw(y, pack, True)
    second = ops.soft_cost_raw(y, pack, True)
    for a, b in zip(first, second):
        assert _same(a, b)
    ref = cost_check(c, dtype_name, *first, f"lin5_eq2 {dtype_name} no LMI")
    n_ineq = int(c.arrays["b1"].size)
    which = first[2].cpu().numpy()
    decided = cost_reference.which_is_decided(ref, cost_reference.bounds(ref, 2.0 ** (-24 if dtype_name == "float32" else -53))[0])
    on_eq = decided & (ref["which"] >= n_ineq)
    assert on_eq.any() and np.array_equal(which[on_eq], ref["which"][on_eq]) and which.max() < ref["vals"].shape[1]
