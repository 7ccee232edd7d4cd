"""method='DC3' on the host: setup against the reference's buffers, the torch formula against its outputs, step counts and
gradients (fixtures: tests/golden/dc3/dc3_*.npz from the real reference), constructor errors, state_dict and pickle."""
import io
import pickle

import numpy as np
import pytest
import torch

import dc3_cases
from rayen_amd import dc3, utils, workloads
from rayen_amd.constraint_module import ConstraintModule


def test_fixtures_cover_the_issue_cases():
    assert {"dc3_cube", "dc3_c2", "dc3_corridor"} <= set(dc3_cases.NAMES)
    assert sum(name.startswith("dc3_example_") for name in dc3_cases.NAMES) >= 8


@pytest.mark.parametrize("name", dc3_cases.NAMES)
def test_setup_matches_the_reference_buffers(name):
    for tag, dtype, bar in (("64", torch.float64, 1e-12), ("32", torch.float32, 2e-6)):
        layer, z = dc3_cases.layer_for(name, dtype)
        assert list(np.asarray(layer.partial_vars)) == list(z["partial_vars"])
        assert list(np.asarray(layer.other_vars)) == list(z["other_vars"])
        assert layer.neq_DC3 == int(z["neq_DC3"]) and layer.dim_after_map == int(z["dim_after_map"]) == layer.n
        for buf in dc3_cases.BUFFERS:
            mine, ref = getattr(layer, buf).numpy(), z[f"buf_{buf}{tag}"]
            assert mine.shape == ref.shape and mine.dtype == ref.dtype, buf
            scale = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
            assert np.all(np.abs(mine - ref) <= bar * scale), (buf, tag)


@pytest.mark.parametrize("name", dc3_cases.NAMES)
def test_rref_pivots_are_the_reference_other_vars(name):
    _, _, z = dc3_cases.load(name)
    if "raw_A2" not in z:
        return
    A2, _ = utils.removeRedundantEquationsFromEqualitySystem(z["raw_A2"], z["raw_b2"])
    _, pivots, _ = utils.rref(A2)
    assert [c for _, c in pivots] == list(z["other_vars"])


@pytest.mark.parametrize("name", dc3_cases.NAMES)
def test_a_state_dict_of_the_reference_buffers_loads(name):
    layer, z = dc3_cases.layer_for(name)
    state = layer.state_dict()
    for buf in dc3_cases.BUFFERS:
        assert buf in state
        state[buf] = torch.tensor(z[f"buf_{buf}32"])
    layer._dc3_packs["stale"] = object()                   # (a pack of the buffers that are about to be replaced)
    layer.load_state_dict(state)
    assert layer._dc3_packs == {}
    layer._dc3_packs["stale"] = object()
    layer.double()
    assert layer._dc3_packs == {}


@pytest.mark.parametrize("mode", dc3_cases.MODES)
@pytest.mark.parametrize("name", dc3_cases.NAMES)
def test_host_formula_reproduces_the_reference(name, mode):
    for tag, dtype, bar in (("64", torch.float64, 1e-11), ("32", torch.float32, 1e-5)):
        layer, z = dc3_cases.layer_for(name, dtype)
        layer.train(mode == "train")
        q = torch.tensor(z["q"]).to(dtype).requires_grad_(True)
        y, steps = dc3.reference_forward(layer, q, return_steps=True)
        assert steps == int(z[f"steps{tag}_{mode}"])
        y_layer = layer(q)
        assert layer.dc3_steps.tolist() == [steps]
        assert torch.equal(y_layer, y) and y.shape == (q.shape[0], layer.k, 1) and y.dtype == dtype
        (torch.tensor(z["w"]).to(dtype).unsqueeze(2) * y_layer).sum().backward()
        assert dc3_cases.row_err(y.detach()[:, :, 0], z[f"y{tag}_{mode}"]).max() <= bar
        assert dc3_cases.row_err(q.grad[:, :, 0], z[f"gq{tag}_{mode}"]).max() <= bar


@pytest.mark.parametrize("name", dc3_cases.NAMES)
def test_recorded_violations_decide_the_step_counts(name):
    """The fixture's fp64 violation after every step, its eps and its step counts agree with the stop rule, and the host
    formula run for a fixed number of steps lands on the recorded violation."""
    layer, z = dc3_cases.layer_for(name, torch.float64)
    _, args, _ = dc3_cases.load(name)
    viol, eps = z["viol64"], args["eps_converge"]
    for mode, limit in (("train", args["max_steps_training"]), ("eval", args["max_steps_testing"])):
        below = [t for t in range(1, limit + 1) if viol[t - 1] < eps]
        assert int(z[f"steps64_{mode}"]) == (below[0] if below else limit)
    layer.eval()
    q = torch.tensor(z["q"]).double()
    for t in (1, 7, len(viol)):
        layer.args_DC3 = dict(args, eps_converge=0.0, max_steps_testing=t)
        y = layer(q)
        stacked = layer.A1_DC3 @ y - layer.b1_DC3
        for i in range(layer.all_P.shape[0]):
            stacked = torch.cat((stacked, 0.5 * y.transpose(1, 2) @ layer.all_P[i] @ y + layer.all_q[i].T @ y
                                 + layer.all_r[i]), dim=1)
        mine = float(torch.relu(stacked).max())
        assert abs(mine - viol[t - 1]) <= 1e-9 * max(1.0, viol[t - 1])


def test_constructor_errors():
    cs = workloads.build_constraints(workloads.cube())
    good = dict(lr=1e-2, momentum=0.5, eps_converge=1e-4, max_steps_training=10, max_steps_testing=50)
    with pytest.raises(NotImplementedError, match="args_DC3") as info:
        ConstraintModule(cs, method="DC3", create_map=False)
    assert isinstance(info.value, RuntimeError)            # what the reference's utils.verify raises
    for key in good:
        with pytest.raises(ValueError, match=key):
            ConstraintModule(cs, method="DC3", create_map=False, args_DC3={k: v for k, v in good.items() if k != key})
    for bad in (float("inf"), 0, -3, 2.5, float("nan"), "10"):
        for key in ("max_steps_training", "max_steps_testing"):
            with pytest.raises(ValueError, match=key):
                ConstraintModule(cs, method="DC3", create_map=False, args_DC3=dict(good, **{key: bad}))
    cones = workloads.build_constraints(workloads.random_lin_quad_soc(k=4, m=6, n_quad=0, n_soc=1, seed=3))
    lmi = workloads.build_constraints(workloads.random_lmi(k=3, r=4, seed=3))
    for other in (cones, lmi):
        with pytest.raises(NotImplementedError):
            ConstraintModule(other, method="DC3", create_map=False, args_DC3=good)
    for method in ("PP", "UP"):
        with pytest.raises(NotImplementedError, match="comparison baselines"):
            ConstraintModule(cs, method=method, create_map=False)
    layer = ConstraintModule(cs, input_dim=5, method="DC3", args_DC3=good)
    assert layer.getDimAfterMap() == 3 and layer.mapper.out_features == 3


def test_pickle_round_trip_and_training_flag():
    layer, z = dc3_cases.layer_for("dc3_corridor")
    layer._dc3_packs["stale"] = object()
    clone = pickle.load(io.BytesIO(pickle.dumps(layer)))
    assert clone._dc3_packs == {} and clone.method == "DC3" and clone.args_DC3 == layer.args_DC3
    assert list(clone.other_vars) == list(layer.other_vars)
    q = torch.tensor(z["q"])
    for training in (True, False):
        layer.train(training)
        clone.train(training)
        assert torch.equal(clone(q), layer(q))
    # the step limit follows self.training: one step in training mode, the fixture's count in eval mode
    layer.args_DC3["max_steps_training"] = 1
    layer.train(True)
    _, steps = dc3.reference_forward(layer, q, return_steps=True)
    assert steps == 1


def test_nan_assertion_names_the_learning_rate():
    layer, z = dc3_cases.layer_for("dc3_cube")
    q = torch.tensor(z["q"]).clone()
    q[3, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"args_DC3\['lr'\]"):
        layer(q)
