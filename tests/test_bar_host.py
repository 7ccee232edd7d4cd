"""method='Bar' on the host: the V-representation (rayen_amd/vrep.py) and the module's construction, formula,
feasibility and checkpoint surface.  No GPU."""
import io
import itertools
import pickle
import warnings

import numpy as np
import pytest
import torch

from helpers import load_golden
from rayen_amd import workloads
from rayen_amd.constraint_module import ConstraintModule
from rayen_amd.vrep import H_to_V

EXPECTED = {"example_00": (3, 0), "example_04": (4, 0), "example_06": (2, 0), "example_07": (1, 4), "example_08": (2, 2)}


def _counts(V, R):
    return V.shape[1], R.shape[1]


def _brute_vertices(A, b):
    """Every feasible point where n linearly independent rows are active, duplicates merged."""
    m, n = A.shape
    out = []
    for rows in itertools.combinations(range(m), n):
        S = A[list(rows)]
        if abs(np.linalg.det(S)) < 1e-9:
            continue
        x = np.linalg.solve(S, b[list(rows)])
        if np.all(A @ x <= b + 1e-9) and not any(np.max(np.abs(x - y)) < 1e-7 for y in out):
            out.append(x)
    return out


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_counts_feasibility_and_extremality_on_the_example_sets(name):
    z = load_golden(name)[2]
    A, b = z["cs_A_p"], z["cs_b_p"].reshape(-1)
    V, R = H_to_V(A, z["cs_b_p"])
    assert _counts(V, R) == EXPECTED[name]
    n = A.shape[1]
    if V.shape[1]:
        assert V.shape[0] == n
    if R.shape[1]:
        assert R.shape[0] == n
    for j in range(V.shape[1]):
        v = V[:, j]
        assert np.all(A @ v <= b + 1e-9)
        active = np.abs(A @ v - b) <= 1e-9
        # n independent active rows on the pointed part (rank A of them where the set has lineality)
        assert (np.linalg.matrix_rank(A[active]) if active.any() else 0) == np.linalg.matrix_rank(A)
    lin = np.linalg.matrix_rank(A) < n
    for j in range(R.shape[1]):
        r = R[:, j]
        assert np.all(A @ r <= 1e-9)
        if not lin:     # extreme: the rows tight on r have rank n - 1
            tight = np.abs(A @ r) <= 1e-9
            assert np.linalg.matrix_rank(A[tight]) == n - 1
    if V.shape[1] == 0:
        assert V.shape == (1, 0)
    if R.shape[1] == 0:
        assert R.shape == (1, 0)


def test_lineality_gives_both_directions():
    V, R = H_to_V(np.zeros((1, 2)), np.ones((1, 1)))       # example 7's filler row: all of R^2
    assert _counts(V, R) == (1, 4)
    assert np.allclose(R[:, :2], -R[:, 2:])
    assert np.allclose(V, 0.0)


@pytest.mark.parametrize("walk", [False, True])
@pytest.mark.parametrize("seed", range(12))
def test_vertices_equal_a_brute_force_enumeration(seed, walk):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 6))
    m = int(rng.integers(n + 1, 21 - 2 * n - 3 * (seed % 3 == 0)))     # at most 20 rows in all
    A = rng.normal(size=(m, n))
    b = rng.uniform(0.2, 1.0, size=m)
    if seed % 3 == 0:
        # degenerate: redundant rows through existing vertices (more than n active rows there), each a positive
        # combination of the rows already active at that vertex
        Ab, bb = np.r_[A, np.eye(n), -np.eye(n)], np.r_[b, np.full(2 * n, 2.0)]
        for x in _brute_vertices(Ab, bb)[:3]:
            act = np.abs(Ab @ x - bb) <= 1e-9
            a = rng.uniform(0.2, 1.0, size=int(act.sum())) @ Ab[act]
            A = np.r_[A, a[None]]
            b = np.r_[b, a @ x]
    A = np.r_[A, np.eye(n), -np.eye(n)]                    # bounded
    b = np.r_[b, np.full(2 * n, 2.0)]
    ref = _brute_vertices(A, b)
    # walk=True: a cap equal to the vertex count sits below the upper-bound theorem's figure for these row counts, so
    # the vertex-graph walk enumerates instead of qhull
    V, R = H_to_V(A, b[:, None], max_generators=len(ref)) if walk else H_to_V(A, b[:, None])
    assert R.shape == (1, 0)
    assert V.shape[1] == len(ref)
    for x in ref:
        assert np.min(np.max(np.abs(V - x[:, None]), axis=0)) < 1e-7


def test_box_and_simplex_counts():
    n = 10
    V, R = H_to_V(np.r_[np.eye(n), -np.eye(n)], np.ones((2 * n, 1)))
    assert _counts(V, R) == (1024, 0)
    n = 64
    V, R = H_to_V(np.r_[-np.eye(n), np.ones((1, n))], np.r_[np.zeros(n), [1.0]][:, None])
    assert _counts(V, R) == (65, 0)


def test_the_cap_applies_to_the_real_generator_count():
    box = np.r_[np.eye(10), -np.eye(10)]
    assert _counts(*H_to_V(box, np.ones((20, 1)), max_generators=1024)) == (1024, 0)
    with pytest.raises(ValueError, match="cap of 1023"):
        H_to_V(box, np.ones((20, 1)), max_generators=1023)
    with pytest.raises(ValueError, match="cap of 3"):
        H_to_V(np.zeros((1, 2)), np.ones((1, 1)), max_generators=3)     # 1 vertex + 4 lineality rays
    n = 17                                                  # a 17-D box: 131 072 vertices, beyond the default cap
    with pytest.raises(ValueError, match="cap of 65536"):
        H_to_V(np.r_[np.eye(n), -np.eye(n)], np.ones((2 * n, 1)))


@pytest.mark.parametrize("touching", [False, True])
def test_many_redundant_rows_and_few_vertices_are_served(touching):
    """Row counts whose upper-bound-theorem figure is far beyond the cap, with few vertices: a 10-D box plus 90
    redundant rows (strictly outside, or through box vertices), and the 8-D cross-polytope (256 facets, 16 vertices)."""
    rng = np.random.default_rng(3)
    D = rng.normal(size=(90, 10))
    A = np.r_[np.eye(10), -np.eye(10), D]
    b = np.r_[np.ones(20), np.abs(D).sum(axis=1) + (0.0 if touching else 0.5)]
    V, R = H_to_V(A, b[:, None])
    assert _counts(V, R) == (1024, 0)
    assert np.allclose(np.abs(V), 1.0, atol=1e-9)
    S = np.array(list(itertools.product([-1.0, 1.0], repeat=8)))
    V, R = H_to_V(S, np.ones((256, 1)))
    assert _counts(V, R) == (16, 0)
    assert np.allclose(np.sort(np.abs(V), axis=0)[-1], 1.0) and np.allclose(np.sort(np.abs(V), axis=0)[:-1], 0.0)


# ---------------------------------------------------------------------------------------------- the module

def _cs(name):
    return workloads.build_constraints(load_golden(name)[0])


def _formula(layer, q):
    """rayen/constraint_module.py:479-486 restated."""
    nv, nr = layer.num_vertices, layer.num_rays
    lam = torch.softmax(q[:, :nv, 0:1], dim=1)
    mu = torch.abs(q[:, nv:nv + nr, 0:1])
    z = torch.zeros(q.shape[0], layer.n, 1, dtype=q.dtype)
    if nv:
        z = z + layer.V.to(q.dtype) @ lam
    if nr:
        z = z + layer.R.to(q.dtype) @ mu
    return layer.NA_E.to(q.dtype) @ z + layer.yp.to(q.dtype)


def test_quadratic_sets_raise_the_reference_message():
    cs = workloads.build_constraints(workloads.random_lin_quad_soc(k=3, m=4, n_quad=1, n_soc=0, seed=1))
    with pytest.raises(Exception, match="Method Bar cannot be used with quadratic constraints"):
        ConstraintModule(cs, method="Bar", create_map=False)


def test_cone_sets_warn_and_keep_the_linear_part():
    cs = workloads.build_constraints(workloads.random_lin_quad_soc(k=3, m=6, n_quad=0, n_soc=1, seed=2))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        layer = ConstraintModule(cs, method="Bar", create_map=False)
    msgs = [str(w.message) for w in caught if issubclass(w.category, UserWarning)]
    assert any("not imposed" in m for m in msgs)
    assert not any(m.startswith("rayen_amd:") for m in msgs)
    assert layer.getDimAfterMap() == layer.num_vertices + layer.num_rays


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_host_forward_equals_the_reference_formula_and_stays_feasible(name):
    cs = _cs(name)
    layer = ConstraintModule(cs, method="Bar", create_map=False).double()
    nv, nr = EXPECTED[name]
    assert (layer.num_vertices, layer.num_rays, layer.getDimAfterMap()) == (nv, nr, nv + nr)
    gen = torch.Generator().manual_seed(0)
    q = torch.empty(10000, nv + nr, 1, dtype=torch.float64).uniform_(-5.0, 5.0, generator=gen)
    y = layer(q)
    assert y.shape == (10000, cs.k, 1) and y.dtype == torch.float64
    assert torch.max(torch.abs(y - _formula(layer, q))).item() <= 1e-12
    z = layer.getzFromy(y)
    A = torch.tensor(cs.A_p, dtype=torch.float64)
    b = torch.tensor(cs.b_p, dtype=torch.float64)
    assert torch.max(A @ z - b).item() <= 1e-9
    # wider inputs: the extra columns are ignored
    wide = torch.cat([q[:50], torch.full((50, 3, 1), 7.0, dtype=torch.float64)], dim=1)
    assert torch.equal(layer(wide), y[:50])


def test_state_dict_permutation_pickle_and_mapper():
    cs = _cs("example_04")
    layer = ConstraintModule(cs, method="Bar", create_map=False).double()
    q = torch.randn(64, layer.getDimAfterMap(), 1, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    y = layer(q)

    other = ConstraintModule(cs, method="Bar", create_map=False).double()
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other(q), y)

    perm = torch.tensor([2, 0, 3, 1])
    state = {k: v.clone() for k, v in layer.state_dict().items()}
    state["V"] = state["V"][:, perm]
    other.load_state_dict(state)
    # column j of the loaded V is old column perm[j]: feeding q's logits in that order gives the old y
    assert torch.allclose(other(q[:, perm]), y, rtol=0, atol=1e-12)
    assert not torch.allclose(other(q), y, rtol=0, atol=1e-6)

    buf = io.BytesIO()
    torch.save(layer, buf)
    buf.seek(0)
    again = torch.load(buf, weights_only=False)
    assert torch.equal(again(q), y)
    assert torch.equal(pickle.loads(pickle.dumps(layer))(q), y)

    mapped = ConstraintModule(cs, input_dim=5, method="Bar", create_map=True).double()
    assert isinstance(mapped.mapper, torch.nn.Linear) and mapped.mapper.out_features == 4
    x = torch.randn(8, 5, 1, dtype=torch.float64, requires_grad=True)
    out = mapped(x)
    out.sum().backward()
    assert out.shape == (8, cs.k, 1) and mapped.mapper.weight.grad is not None and "V" not in dict(mapped.named_parameters())


def test_a_nan_input_asserts_on_the_host():
    layer = ConstraintModule(_cs("example_00"), method="Bar", create_map=False)
    q = torch.zeros(4, 3, 1)
    q[2, 1, 0] = float("nan")
    with pytest.raises(AssertionError):
        layer(q)
