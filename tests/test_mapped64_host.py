"""The fused fp64 mapper (``fuse_mapper64``, include/rayen_hip_mapped64.h) without a device: header, binding and library
agree on the two entry points, their argument checks that need no device, and the module's keyword, its refusal under
another method, old pickles, and host tensors (which never reach the kernel)."""
import os
import pickle
import re

import pytest
import torch

from rayen_amd import _lib, ops, workloads
from rayen_amd.constraint_module import ConstraintModule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BAD_ARG = -1


def _declared():
    text = open(os.path.join(REPO, "include", "rayen_hip_mapped64.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rayen_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_two_entry_points_and_the_main_header_includes_it():
    assert _declared() == ["rayen_mapper_fusable_f64", "rayen_ray_project_mapped_f64"]
    main_header = open(os.path.join(REPO, "include", "rayen_hip.h")).read()
    assert '#include "rayen_hip_mapped64.h"' in main_header
    # (tests/test_abi_load.py counts the symbols of rayen_hip.h itself: the new ones are not declared there)
    stripped = re.sub(r"/\*.*?\*/", "", main_header, flags=re.S)
    assert not any(re.search(r"\b%s\s*\(" % name, stripped) for name in _declared())


def test_binding_header_and_library_agree():
    assert sorted(_lib.EXPORTS_MAPPED64) == _declared()
    others = (_lib.EXPORTS, _lib.EXPORTS_TILE, _lib.EXPORTS_TILE64, _lib.EXPORTS_DC3_TILE, _lib.EXPORTS_DC3_TILE64,
              _lib.EXPORTS_COST_STREAM, _lib.EXPORTS_BAR_STREAM, _lib.EXPORTS_WIDE_FUSED, _lib.EXPORTS_WIDE_FUSED_BWD,
              _lib.EXPORTS_WIDE_FUSED64, _lib.EXPORTS_WIDE_FUSED_BWD64, _lib.EXPORTS_COST_TILE64)
    assert not any(set(_lib.EXPORTS_MAPPED64) & set(o) for o in others)
    lib = _lib.load()
    for name in _lib.EXPORTS_MAPPED64:
        assert hasattr(lib, name), name
    assert lib.rayen_abi_version() == 15


def test_argument_checks_that_need_no_device():
    lib = _lib.load()
    assert lib.rayen_mapper_fusable_f64(None, 8) == 0
    assert lib.rayen_ray_project_mapped_f64(None, None, 0, 8, 8, None, 8, None, None, 0, None, 1, None, None, None,
                                            None) == E_BAD_ARG
    assert lib.rayen_ray_project_mapped_f64(None, None, 4, 8, 8, None, 8, None, None, 0, None, 1, None, None, None,
                                            None) == E_BAD_ARG


def _cs():
    return workloads.build_constraints(workloads.make_raw("c2", seed=41))


def test_keyword_is_accepted_stored_and_off_by_default():
    cs = _cs()
    assert ConstraintModule(cs, input_dim=8, create_map=True).fuse_mapper64 is False
    layer = ConstraintModule(cs, input_dim=8, create_map=True, fuse_mapper64=True)
    assert layer.fuse_mapper64 is True and layer.fuse_mapper is True
    with pytest.raises(TypeError):
        ConstraintModule(cs, 8, 'RAYEN', True, None, True)          # keyword-only
    assert hasattr(ops, "mapper_fusable64") and hasattr(torch.ops.rayen_amd, "ray_project_mapped64")


def test_another_method_refuses_the_keyword():
    with pytest.raises(ValueError, match="fuse_mapper64.*method 'RAYEN'.*'Bar'"):
        ConstraintModule(_cs(), input_dim=8, method='Bar', create_map=True, fuse_mapper64=True)
    lin = workloads.build_constraints(workloads.make_raw("c1"))          # (a set method 'Bar' takes: the keyword is the cause)
    assert ConstraintModule(lin, input_dim=8, method='Bar', create_map=True, fuse_mapper64=False).fuse_mapper64 is False
    with pytest.raises(ValueError, match="fuse_mapper64"):
        ConstraintModule(lin, input_dim=8, method='Bar', create_map=True, fuse_mapper64=True)


def test_old_pickles_load_with_the_route_off():
    layer = ConstraintModule(_cs(), input_dim=8, create_map=True, fuse_mapper64=True)
    assert pickle.loads(pickle.dumps(layer)).fuse_mapper64 is True
    state = layer.__getstate__()
    del state["fuse_mapper64"]                                       # a pickle from before the keyword
    old = ConstraintModule.__new__(ConstraintModule)
    old.__setstate__(state)
    assert old.fuse_mapper64 is False


def test_host_tensors_never_reach_the_kernel():
    cs = _cs()
    outs = []
    for fuse in (False, True):
        torch.manual_seed(0)
        layer = ConstraintModule(cs, input_dim=8, create_map=True, fuse_mapper64=fuse).double()
        x = torch.empty(37, 8, 1, dtype=torch.float64).uniform_(-2.0, 2.0, generator=torch.Generator().manual_seed(3))
        x.requires_grad_(True)
        y = layer(x)
        y.sum().backward()
        outs.append((y.detach(), x.grad, layer.mapper.weight.grad))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    w = torch.zeros(cs.n, 8, dtype=torch.float64)
    assert ops.mapper_fusable64(torch.zeros(3, 8, dtype=torch.float64), w, None, None) is False
