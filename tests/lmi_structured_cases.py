"""Seeded LMIs with STRUCTURE, their rows and their fp64 truth, shared by tests/test_lmi_structured_host.py and
tests/test_gpu_lmi_structured.py.

Every other LMI in the suite has dense uniform generators ``(T + T') / 2``: no Householder column is ever (nearly) zero,
the top eigenvalue is always well separated and every entry is O(1).  The cases here are what users write instead.

Conventions.  A case is a raw dict in the format of ``workloads._empty(k)`` with ``y0 = 0`` and ``F[k] = I``: the
reference's Cholesky factor is then exactly ``I`` and the matrix the kernels take the largest eigenvalue of is
``S(v) = -sum_a v_a F_a``.  All generators of a case share the structure, so ``S(v)`` has it for every ``v``.

Structures (:data:`CASES` lists every instance by name):
  * ``diag``       ``F_a = diag(d_a)``: linear rows in disguise -- ``I + sum y_a diag(d_a) >= 0`` is ``A1 y <= b1`` with
                   ``A1 = -D'`` (``D [k, r]`` the diagonals) and ``b1 = 1`` (:func:`polytope_raw`);
  * ``tridiag``    random tridiagonal generators: every Householder step has nothing to annihilate;
  * ``toeplitz``   k = 1, ``F_1 = tridiag(-1, 2, -1)``: the set is ``y >= -1 / (2 + 2 cos(pi / (r + 1)))``;
  * ``blockdiag``  two dense random blocks ``p + q`` (block edges off a multiple of 4; the top eigenvalue sits in either
                   block, depending on the row; a block of 1 is a zero column in front or a zero row at the end);
  * ``zero_line``  row and column ``j`` zero in every generator (``j`` = 0, the middle, r - 1);
  * ``arrow``      a diagonal plus the first row and column;
  * ``rank_one``   ``F_a = u_a u_a'``: r - k zero eigenvalues, and rows with ``S < 0`` (kappa = 0);
  * ``identity``   k = 1, ``F_1 = I``: all eigenvalues tie, the set is ``y >= -1``; ``identity2`` adds
                   ``F_2 = diag(0 .. r - 1) / r``;
  * ``twin``       two blocks ``[[0, c], [c, 0]]`` on four consecutive indices, coupled by ONE entry ``delta`` between the
                   first and the last of them: the top pair is ``c +- delta / 2``, so an eigen-solver that loses ``delta``
                   is off by ``delta / 2c`` in the first order.  The second generator is ``diag(d_tail)`` on the other
                   indices, ``d_tail`` in [0.1, 0.5].  ``delta / c`` is 1e-4 (fp32) or 7e-9 (fp64) -- ``delta^2`` is below the
                   half-ulp of ``c^2`` in every binade, so a sum of squares that includes ``c^2`` does not see it -- and
                   1e-2 / 1e-5 as controls; ``at``: the first of the four indices, ``rev``: indices reversed;
  * ``wilkinson``  k = 1, ``W_21^+`` (diagonal |10 .. 0 .. 10|, off-diagonal 1) in the middle of a zero matrix: its top
                   pair agrees to about 1e-14;
  * ``graded``     ``D W_a D`` with ``D = diag(10^(-p i / r))``, p = 3 (fp32) or 6 (fp64);
  * ``scaled``     dense random generators times 1e-4 / 1e4 (fp32) or 1e-8 / 1e8 (fp64).

Rows (:func:`rows`): B = 64 for r <= 66 and 16 beyond, uniform(-2, 2) rounded to fp32 (both precisions read the same
numbers); rows 0-1 times 1e-4 (interior), row 2 zero, the next 2k rows ``+-e_a`` (``S`` is a single generator).

Truth (:func:`truth`): ``oracle.forward`` in fp64; ``kappa`` and the top-pair gap from ``oracle.compute_kappa(...,
terms=True)``, as in tests/test_gpu_lmi_wave.py::_check_backward.  :func:`kinks` restates that function's rule on the
fp64 reference alone.

:data:`TABLE` is the literal list of (case, kernel family, precision) the device tests run; :data:`BACKWARD_SEPARATED`
and :data:`BACKWARD_TIED` are the subsets with a gradient check.  tests/test_lmi_structured_host.py proves every case
well-posed on the CPU before a kernel sees it.
"""
import functools

import numpy as np
import torch

from helpers import csd_from_cs
from oracle import rayen_oracle as oracle
from rayen_amd import workloads
from rayen_amd.soft_cost import set_arrays

import cost_lmi_cases

TWIN_C = 2.0
BAR = {"float32": 1e-5, "float64": 1e-9}          # the project's forward bars (relative, per row)
GAP = {"float32": 1e-3, "float64": 1e-7}          # tests/test_gpu_lmi_wave.py::_check_backward: a smaller gap is a kink


def _sym(rng, r):
    T = rng.uniform(-1.0, 1.0, size=(r, r))
    return (T + T.T) / 2


def _raw(F):
    r = F[0].shape[0]
    raw = workloads._empty(len(F))
    raw["F"] = [np.array(Fa, dtype=np.float64) for Fa in F] + [np.eye(r)]
    return raw


def diag(r, seed, k=3):
    rng = np.random.default_rng(seed)
    return _raw([np.diag(rng.uniform(-1.0, 1.0, size=r)) for _ in range(k)])


def polytope_raw(raw):
    """The diagonal LMI ``raw`` as linear rows: ``A1 = -D'``, ``b1 = 1``."""
    D = np.stack([np.diag(Fa) for Fa in raw["F"][:-1]], axis=0)          # [k, r]
    out = workloads._empty(D.shape[0])
    out["A1"], out["b1"] = -D.T.copy(), np.ones((D.shape[1], 1))
    return out


def tridiag(r, seed, k=3):
    rng = np.random.default_rng(seed)
    F = []
    for _ in range(k):
        e = rng.uniform(-1.0, 1.0, size=max(r - 1, 0))
        F.append(np.diag(rng.uniform(-1.0, 1.0, size=r)) + np.diag(e, 1) + np.diag(e, -1))
    return _raw(F)


def toeplitz(r):
    e = -np.ones(r - 1)
    return _raw([2.0 * np.eye(r) + np.diag(e, 1) + np.diag(e, -1)])


def toeplitz_bound(r):
    return -1.0 / (2.0 + 2.0 * np.cos(np.pi / (r + 1)))


def blockdiag(p, q, seed, k=3):
    rng = np.random.default_rng(seed)
    F = []
    for _ in range(k):
        Fa = np.zeros((p + q, p + q))
        Fa[:p, :p], Fa[p:, p:] = _sym(rng, p), _sym(rng, q)
        F.append(Fa)
    return _raw(F)


def zero_line(r, j, seed, k=3):
    rng = np.random.default_rng(seed)
    F = []
    for _ in range(k):
        Fa = _sym(rng, r)
        Fa[j, :] = 0.0
        Fa[:, j] = 0.0
        F.append(Fa)
    return _raw(F)


def arrow(r, seed, k=3):
    rng = np.random.default_rng(seed)
    F = []
    for _ in range(k):
        Fa = np.diag(rng.uniform(-1.0, 1.0, size=r))
        row = rng.uniform(-1.0, 1.0, size=r - 1)
        Fa[0, 1:], Fa[1:, 0] = row, row
        F.append(Fa)
    return _raw(F)


def rank_one(r, seed, k=3):
    rng = np.random.default_rng(seed)
    return _raw([np.outer(u, u) for u in rng.uniform(-1.0, 1.0, size=(k, r))])


def identity(r, k=1):
    F = [np.eye(r)]
    if k == 2:
        F.append(np.diag(np.arange(r) / r))
    return _raw(F)


def twin(r, at, ratio, rev, seed):
    rng = np.random.default_rng(seed)
    c, delta = TWIN_C, TWIN_C * ratio
    M = np.zeros((r, r))
    for a, b, val in ((at, at + 1, c), (at + 2, at + 3, c), (at, at + 3, delta)):
        M[a, b] = M[b, a] = val
    tail = rng.uniform(0.1, 0.5, size=r)
    tail[at:at + 4] = 0.0
    F = [M, np.diag(tail)]
    if rev:
        F = [Fa[::-1, ::-1].copy() for Fa in F]
    return _raw(F)


def twin_without_delta(raw):
    """The same case with the coupling entries (the two smallest nonzero entries of the first generator) zeroed."""
    out = dict(raw, F=[Fa.copy() for Fa in raw["F"]])
    M = out["F"][0]
    M[np.abs(M) < 0.5 * TWIN_C] = 0.0
    return out


def wilkinson(r):
    W = np.diag(np.abs(np.arange(21) - 10.0)) + np.diag(np.ones(20), 1) + np.diag(np.ones(20), -1)
    F = np.zeros((r, r))
    o = (r - 21) // 2
    F[o:o + 21, o:o + 21] = W
    return _raw([F])


def graded(r, p, seed, k=3):
    rng = np.random.default_rng(seed)
    d = 10.0 ** (-p * np.arange(r) / r)
    return _raw([_sym(rng, r) * np.outer(d, d) for _ in range(k)])


def scaled(r, scale, seed, k=3):
    rng = np.random.default_rng(seed)
    return _raw([scale * _sym(rng, r) for _ in range(k)])


# name -> (builder, arguments).  Seeds are chosen so that the kink cap of the gradient cases holds and LAPACK's fp32
# arithmetic stays within 2e-6 of the truth (tests/test_lmi_structured_host.py: test_kink_cap_of_the_gradient_cases,
# test_lapack_fp32_is_far_inside_the_fp32_bar).
CASES = {
    "diag_r1": (diag, dict(r=1, seed=101)), "diag_r2": (diag, dict(r=2, seed=102)), "diag_r3": (diag, dict(r=3, seed=103)),
    "diag_r4": (diag, dict(r=4, seed=104)), "diag_r5": (diag, dict(r=5, seed=105)), "diag_r8": (diag, dict(r=8, seed=108)),
    "diag_r9": (diag, dict(r=9, seed=109)),
    "diag_r16": (diag, dict(r=16, seed=116)), "diag_r17": (diag, dict(r=17, seed=117)), "diag_r32": (diag, dict(r=32, seed=132)),
    "diag_r25": (diag, dict(r=25, seed=125)), "diag_r44": (diag, dict(r=44, seed=144)), "diag_r33": (diag, dict(r=33, seed=133)),
    "diag_r64": (diag, dict(r=64, seed=164)), "diag_r45": (diag, dict(r=45, seed=145)), "diag_r65": (diag, dict(r=65, seed=165)),
    "diag_r66": (diag, dict(r=66, seed=166)), "diag_r129": (diag, dict(r=129, seed=229)),
    "tridiag_r2": (tridiag, dict(r=2, seed=202)), "tridiag_r3": (tridiag, dict(r=3, seed=203)),
    "tridiag_r4": (tridiag, dict(r=4, seed=206)), "tridiag_r5": (tridiag, dict(r=5, seed=205)),
    "tridiag_r9": (tridiag, dict(r=9, seed=209)), "tridiag_r16": (tridiag, dict(r=16, seed=216)),
    "tridiag_r17": (tridiag, dict(r=17, seed=217)), "tridiag_r32": (tridiag, dict(r=32, seed=232)),
    "tridiag_r25": (tridiag, dict(r=25, seed=225)), "tridiag_r44": (tridiag, dict(r=44, seed=244)),
    "tridiag_r33": (tridiag, dict(r=33, seed=233)), "tridiag_r64": (tridiag, dict(r=64, seed=264)),
    "tridiag_r45": (tridiag, dict(r=45, seed=245)), "tridiag_r65": (tridiag, dict(r=65, seed=265)),
    "tridiag_r66": (tridiag, dict(r=66, seed=266)), "tridiag_r129": (tridiag, dict(r=129, seed=329)),
    "toeplitz_r5": (toeplitz, dict(r=5)), "toeplitz_r16": (toeplitz, dict(r=16)), "toeplitz_r32": (toeplitz, dict(r=32)),
    "toeplitz_r25": (toeplitz, dict(r=25)), "toeplitz_r44": (toeplitz, dict(r=44)), "toeplitz_r33": (toeplitz, dict(r=33)),
    "toeplitz_r64": (toeplitz, dict(r=64)), "toeplitz_r45": (toeplitz, dict(r=45)), "toeplitz_r65": (toeplitz, dict(r=65)),
    "toeplitz_r66": (toeplitz, dict(r=66)),
    "blockdiag_3_2": (blockdiag, dict(p=3, q=2, seed=301)), "blockdiag_5_4": (blockdiag, dict(p=5, q=4, seed=302)),
    "blockdiag_9_7": (blockdiag, dict(p=9, q=7, seed=303)), "blockdiag_10_7": (blockdiag, dict(p=10, q=7, seed=304)),
    "blockdiag_19_13": (blockdiag, dict(p=19, q=13, seed=305)), "blockdiag_14_11": (blockdiag, dict(p=14, q=11, seed=306)),
    "blockdiag_25_19": (blockdiag, dict(p=25, q=19, seed=307)), "blockdiag_19_14": (blockdiag, dict(p=19, q=14, seed=308)),
    "blockdiag_1_32": (blockdiag, dict(p=1, q=32, seed=309)), "blockdiag_32_1": (blockdiag, dict(p=32, q=1, seed=310)),
    "blockdiag_33_31": (blockdiag, dict(p=33, q=31, seed=311)), "blockdiag_33_32": (blockdiag, dict(p=33, q=32, seed=312)),
    "blockdiag_41_25": (blockdiag, dict(p=41, q=25, seed=313)), "blockdiag_19_26": (blockdiag, dict(p=19, q=26, seed=314)),
    "blockdiag_66_63": (blockdiag, dict(p=66, q=63, seed=315)), "blockdiag_150_132": (blockdiag, dict(p=150, q=132, seed=316)),
    "zero_line_r5_j0": (zero_line, dict(r=5, j=0, seed=401)), "zero_line_r9_j4": (zero_line, dict(r=9, j=4, seed=402)),
    "zero_line_r16_j8": (zero_line, dict(r=16, j=8, seed=403)), "zero_line_r17_j16": (zero_line, dict(r=17, j=16, seed=404)),
    "zero_line_r32_j0": (zero_line, dict(r=32, j=0, seed=405)), "zero_line_r25_j12": (zero_line, dict(r=25, j=12, seed=406)),
    "zero_line_r44_j43": (zero_line, dict(r=44, j=43, seed=407)), "zero_line_r33_j0": (zero_line, dict(r=33, j=0, seed=408)),
    "zero_line_r64_j32": (zero_line, dict(r=64, j=32, seed=409)), "zero_line_r65_j64": (zero_line, dict(r=65, j=64, seed=410)),
    "zero_line_r66_j0": (zero_line, dict(r=66, j=0, seed=416)), "zero_line_r45_j22": (zero_line, dict(r=45, j=22, seed=412)),
    "zero_line_r129_j128": (zero_line, dict(r=129, j=128, seed=413)),
    "arrow_r2": (arrow, dict(r=2, seed=502)), "arrow_r3": (arrow, dict(r=3, seed=503)), "arrow_r4": (arrow, dict(r=4, seed=506)),
    "arrow_r5": (arrow, dict(r=5, seed=505)), "arrow_r9": (arrow, dict(r=9, seed=509)), "arrow_r16": (arrow, dict(r=16, seed=516)),
    "arrow_r17": (arrow, dict(r=17, seed=517)), "arrow_r32": (arrow, dict(r=32, seed=532)), "arrow_r25": (arrow, dict(r=25, seed=525)),
    "arrow_r44": (arrow, dict(r=44, seed=544)), "arrow_r33": (arrow, dict(r=33, seed=533)), "arrow_r64": (arrow, dict(r=64, seed=564)),
    "arrow_r45": (arrow, dict(r=45, seed=545)), "arrow_r65": (arrow, dict(r=65, seed=565)), "arrow_r66": (arrow, dict(r=66, seed=566)),
    "arrow_r129": (arrow, dict(r=129, seed=629)),
    "rank_one_r4": (rank_one, dict(r=4, seed=604)), "rank_one_r5": (rank_one, dict(r=5, seed=605)),
    "rank_one_r16": (rank_one, dict(r=16, seed=616)), "rank_one_r17": (rank_one, dict(r=17, seed=617)),
    "rank_one_r32": (rank_one, dict(r=32, seed=632)), "rank_one_r25": (rank_one, dict(r=25, seed=625)),
    "rank_one_r44": (rank_one, dict(r=44, seed=644)), "rank_one_r33": (rank_one, dict(r=33, seed=633)),
    "rank_one_r64": (rank_one, dict(r=64, seed=664)), "rank_one_r45": (rank_one, dict(r=45, seed=645)),
    "rank_one_r65": (rank_one, dict(r=65, seed=665)), "rank_one_r66": (rank_one, dict(r=66, seed=666)),
    "rank_one_r129": (rank_one, dict(r=129, seed=729)),
    "identity_r1": (identity, dict(r=1)), "identity_r2": (identity, dict(r=2)), "identity_r4": (identity, dict(r=4)),
    "identity_r5": (identity, dict(r=5)), "identity_r16": (identity, dict(r=16)), "identity_r17": (identity, dict(r=17)),
    "identity_r32": (identity, dict(r=32)), "identity_r25": (identity, dict(r=25)), "identity_r44": (identity, dict(r=44)),
    "identity_r33": (identity, dict(r=33)), "identity_r64": (identity, dict(r=64)), "identity_r45": (identity, dict(r=45)),
    "identity_r65": (identity, dict(r=65)), "identity_r66": (identity, dict(r=66)),
    "identity2_r5": (identity, dict(r=5, k=2)), "identity2_r16": (identity, dict(r=16, k=2)),
    "identity2_r32": (identity, dict(r=32, k=2)), "identity2_r25": (identity, dict(r=25, k=2)),
    "identity2_r44": (identity, dict(r=44, k=2)), "identity2_r33": (identity, dict(r=33, k=2)),
    "identity2_r64": (identity, dict(r=64, k=2)), "identity2_r45": (identity, dict(r=45, k=2)),
    "identity2_r65": (identity, dict(r=65, k=2)), "identity2_r66": (identity, dict(r=66, k=2)),
    # twin: ratio 1e-4 (fp32) / 7e-9 (fp64), controls 1e-2 and 1e-5
    "twin_r5_1e-4": (twin, dict(r=5, at=0, ratio=1e-4, rev=False, seed=701)),
    "twin_r5_1e-4_rev": (twin, dict(r=5, at=0, ratio=1e-4, rev=True, seed=701)),
    "twin_r8_1e-4": (twin, dict(r=8, at=0, ratio=1e-4, rev=False, seed=702)),
    "twin_r16_1e-4": (twin, dict(r=16, at=0, ratio=1e-4, rev=False, seed=703)),
    "twin_r16_1e-4_rev": (twin, dict(r=16, at=0, ratio=1e-4, rev=True, seed=703)),
    "twin_r17_1e-4": (twin, dict(r=17, at=0, ratio=1e-4, rev=False, seed=704)),
    "twin_r32_1e-4_rev": (twin, dict(r=32, at=0, ratio=1e-4, rev=True, seed=705)),
    "twin_r33_1e-4": (twin, dict(r=33, at=0, ratio=1e-4, rev=False, seed=706)),
    "twin_r33_1e-4_rev": (twin, dict(r=33, at=0, ratio=1e-4, rev=True, seed=706)),
    "twin_r33_1e-2": (twin, dict(r=33, at=0, ratio=1e-2, rev=False, seed=706)),
    "twin_r33_1e-5": (twin, dict(r=33, at=0, ratio=1e-5, rev=False, seed=706)),
    "twin_r64_1e-4": (twin, dict(r=64, at=0, ratio=1e-4, rev=False, seed=707)),
    "twin_r64_1e-4_rev": (twin, dict(r=64, at=0, ratio=1e-4, rev=True, seed=707)),
    "twin_r66_at40_1e-4": (twin, dict(r=66, at=40, ratio=1e-4, rev=False, seed=708)),
    "twin_r66_at40_1e-4_rev": (twin, dict(r=66, at=40, ratio=1e-4, rev=True, seed=708)),
    "twin_r129_1e-4": (twin, dict(r=129, at=0, ratio=1e-4, rev=False, seed=709)),
    "twin_r129_1e-4_rev": (twin, dict(r=129, at=0, ratio=1e-4, rev=True, seed=709)),
    "twin_r282_at8_1e-4": (twin, dict(r=282, at=8, ratio=1e-4, rev=False, seed=710)),
    "twin_r282_at8_1e-4_rev": (twin, dict(r=282, at=8, ratio=1e-4, rev=True, seed=710)),
    "twin_r282_at100_1e-4": (twin, dict(r=282, at=100, ratio=1e-4, rev=False, seed=711)),
    "twin_r282_at100_1e-4_rev": (twin, dict(r=282, at=100, ratio=1e-4, rev=True, seed=711)),
    "twin_r5_7e-9": (twin, dict(r=5, at=0, ratio=7e-9, rev=False, seed=721)),
    "twin_r5_7e-9_rev": (twin, dict(r=5, at=0, ratio=7e-9, rev=True, seed=721)),
    "twin_r8_7e-9": (twin, dict(r=8, at=0, ratio=7e-9, rev=False, seed=722)),
    "twin_r16_7e-9": (twin, dict(r=16, at=0, ratio=7e-9, rev=False, seed=723)),
    "twin_r16_7e-9_rev": (twin, dict(r=16, at=0, ratio=7e-9, rev=True, seed=723)),
    "twin_r17_7e-9": (twin, dict(r=17, at=0, ratio=7e-9, rev=False, seed=724)),
    "twin_r25_7e-9": (twin, dict(r=25, at=0, ratio=7e-9, rev=False, seed=725)),
    "twin_r25_7e-9_rev": (twin, dict(r=25, at=0, ratio=7e-9, rev=True, seed=725)),
    "twin_r44_7e-9": (twin, dict(r=44, at=0, ratio=7e-9, rev=False, seed=726)),
    "twin_r44_7e-9_rev": (twin, dict(r=44, at=0, ratio=7e-9, rev=True, seed=726)),
    "twin_r44_1e-2": (twin, dict(r=44, at=0, ratio=1e-2, rev=False, seed=726)),
    "twin_r44_1e-5": (twin, dict(r=44, at=0, ratio=1e-5, rev=False, seed=726)),
    "twin_r45_7e-9": (twin, dict(r=45, at=0, ratio=7e-9, rev=False, seed=727)),
    "twin_r45_7e-9_rev": (twin, dict(r=45, at=0, ratio=7e-9, rev=True, seed=727)),
    "twin_r45_1e-2": (twin, dict(r=45, at=0, ratio=1e-2, rev=False, seed=727)),
    "twin_r45_1e-5": (twin, dict(r=45, at=0, ratio=1e-5, rev=False, seed=727)),
    "twin_r65_at40_7e-9": (twin, dict(r=65, at=40, ratio=7e-9, rev=False, seed=728)),
    "twin_r65_at40_7e-9_rev": (twin, dict(r=65, at=40, ratio=7e-9, rev=True, seed=728)),
    "twin_r129_7e-9": (twin, dict(r=129, at=0, ratio=7e-9, rev=False, seed=729)),
    "twin_r129_7e-9_rev": (twin, dict(r=129, at=0, ratio=7e-9, rev=True, seed=729)),
    "wilkinson_r32": (wilkinson, dict(r=32)), "wilkinson_r25": (wilkinson, dict(r=25)), "wilkinson_r44": (wilkinson, dict(r=44)),
    "wilkinson_r33": (wilkinson, dict(r=33)), "wilkinson_r64": (wilkinson, dict(r=64)), "wilkinson_r45": (wilkinson, dict(r=45)),
    "wilkinson_r65": (wilkinson, dict(r=65)), "wilkinson_r66": (wilkinson, dict(r=66)),
    "graded3_r5": (graded, dict(r=5, p=3, seed=805)), "graded3_r16": (graded, dict(r=16, p=3, seed=816)),
    "graded3_r17": (graded, dict(r=17, p=3, seed=817)), "graded3_r32": (graded, dict(r=32, p=3, seed=832)),
    "graded3_r33": (graded, dict(r=33, p=3, seed=833)), "graded3_r64": (graded, dict(r=64, p=3, seed=864)),
    "graded3_r66": (graded, dict(r=66, p=3, seed=866)), "graded3_r129": (graded, dict(r=129, p=3, seed=929)),
    "graded6_r5": (graded, dict(r=5, p=6, seed=905)), "graded6_r16": (graded, dict(r=16, p=6, seed=916)),
    "graded6_r17": (graded, dict(r=17, p=6, seed=917)), "graded6_r25": (graded, dict(r=25, p=6, seed=925)),
    "graded6_r44": (graded, dict(r=44, p=6, seed=944)), "graded6_r45": (graded, dict(r=45, p=6, seed=945)),
    "graded6_r65": (graded, dict(r=65, p=6, seed=965)), "graded6_r129": (graded, dict(r=129, p=6, seed=1029)),
    "scaled_r5_1e-4": (scaled, dict(r=5, scale=1e-4, seed=1105)), "scaled_r16_1e4": (scaled, dict(r=16, scale=1e4, seed=1116)),
    "scaled_r33_1e-4": (scaled, dict(r=33, scale=1e-4, seed=1133)), "scaled_r64_1e4": (scaled, dict(r=64, scale=1e4, seed=1170)),
    "scaled_r66_1e4": (scaled, dict(r=66, scale=1e4, seed=1171)),
    "scaled_r5_1e-8": (scaled, dict(r=5, scale=1e-8, seed=1205)), "scaled_r16_1e8": (scaled, dict(r=16, scale=1e8, seed=1216)),
    "scaled_r25_1e-8": (scaled, dict(r=25, scale=1e-8, seed=1225)), "scaled_r44_1e8": (scaled, dict(r=44, scale=1e8, seed=1244)),
    "scaled_r45_1e-8": (scaled, dict(r=45, scale=1e-8, seed=1245)), "scaled_r65_1e8": (scaled, dict(r=65, scale=1e8, seed=1265)),
}

# (kernel family, precision) -> the cases it runs.  quad: the default below 33 x 33 (fp32) / 25 x 25 (fp64) -- a 1 x 1
# matrix is not the quad kernel's (rayen_lmi_quad.h: r >= 2), the default sends it to the lane kernel, and FAMILY_OF says
# so; lane: force_generic=True; wave / block: RAYEN_LMI_BLOCK = 0 / 1.
TABLE = {
    ("quad", "float32"): """diag_r1 diag_r2 diag_r3 diag_r4 diag_r5 diag_r9 diag_r16 diag_r17 diag_r32
        tridiag_r2 tridiag_r3 tridiag_r4 tridiag_r5 tridiag_r9 tridiag_r16 tridiag_r17 tridiag_r32 toeplitz_r5 toeplitz_r32
        blockdiag_3_2 blockdiag_5_4 blockdiag_9_7 blockdiag_10_7 blockdiag_19_13
        zero_line_r5_j0 zero_line_r9_j4 zero_line_r16_j8 zero_line_r17_j16 zero_line_r32_j0
        arrow_r2 arrow_r3 arrow_r4 arrow_r5 arrow_r9 arrow_r16 arrow_r17 arrow_r32
        rank_one_r4 rank_one_r5 rank_one_r16 rank_one_r17 rank_one_r32
        identity_r1 identity_r2 identity_r4 identity_r5 identity_r16 identity_r17 identity_r32 identity2_r5 identity2_r32
        twin_r5_1e-4 twin_r5_1e-4_rev twin_r16_1e-4 twin_r16_1e-4_rev twin_r17_1e-4 twin_r32_1e-4_rev
        wilkinson_r32 graded3_r5 graded3_r16 graded3_r17 graded3_r32 scaled_r5_1e-4 scaled_r16_1e4""",
    ("quad", "float64"): """diag_r1 diag_r2 diag_r3 diag_r4 diag_r5 diag_r9 diag_r16 diag_r17
        tridiag_r2 tridiag_r3 tridiag_r4 tridiag_r5 tridiag_r9 tridiag_r16 tridiag_r17 toeplitz_r5 toeplitz_r16
        blockdiag_3_2 blockdiag_5_4 blockdiag_9_7 blockdiag_10_7
        zero_line_r5_j0 zero_line_r9_j4 zero_line_r16_j8 zero_line_r17_j16
        arrow_r2 arrow_r3 arrow_r4 arrow_r5 arrow_r9 arrow_r16 arrow_r17
        rank_one_r4 rank_one_r5 rank_one_r16 rank_one_r17
        identity_r1 identity_r2 identity_r4 identity_r5 identity_r16 identity_r17 identity2_r5 identity2_r16
        twin_r5_7e-9 twin_r5_7e-9_rev twin_r16_7e-9 twin_r16_7e-9_rev twin_r17_7e-9
        graded6_r5 graded6_r16 graded6_r17 scaled_r5_1e-8 scaled_r16_1e8""",
    ("lane", "float32"): """diag_r2 diag_r5 diag_r16 tridiag_r2 tridiag_r5 tridiag_r16 toeplitz_r5 toeplitz_r16
        blockdiag_3_2 blockdiag_9_7 zero_line_r5_j0 zero_line_r16_j8 arrow_r2 arrow_r5 arrow_r16 rank_one_r5 rank_one_r16
        identity_r2 identity_r5 identity_r16 identity2_r5 identity2_r16 twin_r5_1e-4 twin_r5_1e-4_rev twin_r16_1e-4
        twin_r16_1e-4_rev graded3_r5 graded3_r16 scaled_r5_1e-4 scaled_r16_1e4""",
    ("lane", "float64"): """diag_r2 diag_r5 diag_r16 tridiag_r2 tridiag_r5 tridiag_r16 toeplitz_r5 toeplitz_r16
        blockdiag_3_2 blockdiag_9_7 zero_line_r5_j0 zero_line_r16_j8 arrow_r2 arrow_r5 arrow_r16 rank_one_r5 rank_one_r16
        identity_r2 identity_r5 identity_r16 identity2_r5 identity2_r16 twin_r5_7e-9 twin_r5_7e-9_rev twin_r16_7e-9
        twin_r16_7e-9_rev graded6_r5 graded6_r16 scaled_r5_1e-8 scaled_r16_1e8""",
    ("wave", "float32"): """diag_r33 diag_r64 tridiag_r33 tridiag_r64 toeplitz_r33 toeplitz_r64
        blockdiag_19_14 blockdiag_1_32 blockdiag_32_1 blockdiag_33_31 blockdiag_33_32
        zero_line_r33_j0 zero_line_r64_j32 zero_line_r65_j64 arrow_r33 arrow_r64 rank_one_r33 rank_one_r64
        identity_r33 identity_r64 identity2_r33 identity2_r64
        twin_r33_1e-4 twin_r33_1e-4_rev twin_r33_1e-2 twin_r33_1e-5 twin_r64_1e-4 twin_r64_1e-4_rev
        wilkinson_r33 wilkinson_r64 graded3_r33 graded3_r64 scaled_r33_1e-4 scaled_r64_1e4""",
    ("wave", "float64"): """diag_r25 diag_r44 tridiag_r25 tridiag_r44 toeplitz_r25 toeplitz_r44
        blockdiag_14_11 blockdiag_25_19 zero_line_r25_j12 zero_line_r44_j43 arrow_r25 arrow_r44 rank_one_r25 rank_one_r44
        identity_r25 identity_r44 identity2_r25 identity2_r44
        twin_r25_7e-9 twin_r25_7e-9_rev twin_r44_7e-9 twin_r44_7e-9_rev twin_r44_1e-2 twin_r44_1e-5
        wilkinson_r25 wilkinson_r44 graded6_r25 graded6_r44 scaled_r25_1e-8 scaled_r44_1e8""",
    ("block", "float32"): """diag_r33 diag_r66 diag_r129 tridiag_r33 tridiag_r66 tridiag_r129 toeplitz_r33 toeplitz_r66
        blockdiag_19_14 blockdiag_1_32 blockdiag_32_1 blockdiag_33_32 blockdiag_41_25 blockdiag_66_63 blockdiag_150_132
        zero_line_r33_j0 zero_line_r65_j64 zero_line_r66_j0 zero_line_r129_j128 arrow_r33 arrow_r66 arrow_r129
        rank_one_r33 rank_one_r66 rank_one_r129 identity_r33 identity_r66 identity2_r33 identity2_r66
        twin_r33_1e-4 twin_r33_1e-4_rev twin_r33_1e-2 twin_r33_1e-5 twin_r66_at40_1e-4 twin_r66_at40_1e-4_rev
        twin_r129_1e-4 twin_r129_1e-4_rev twin_r282_at8_1e-4 twin_r282_at8_1e-4_rev twin_r282_at100_1e-4
        twin_r282_at100_1e-4_rev wilkinson_r33 wilkinson_r66 graded3_r33 graded3_r66 graded3_r129
        scaled_r33_1e-4 scaled_r66_1e4""",
    ("block", "float64"): """diag_r45 diag_r65 diag_r129 tridiag_r45 tridiag_r65 tridiag_r129 toeplitz_r45 toeplitz_r65
        blockdiag_19_26 blockdiag_33_32 blockdiag_66_63 zero_line_r45_j22 zero_line_r65_j64 zero_line_r129_j128
        arrow_r45 arrow_r65 arrow_r129 rank_one_r45 rank_one_r65 rank_one_r129
        identity_r45 identity_r65 identity2_r45 identity2_r65
        twin_r45_7e-9 twin_r45_7e-9_rev twin_r45_1e-2 twin_r45_1e-5 twin_r65_at40_7e-9 twin_r65_at40_7e-9_rev
        twin_r129_7e-9 twin_r129_7e-9_rev wilkinson_r45 wilkinson_r65 graded6_r45 graded6_r65 graded6_r129
        scaled_r45_1e-8 scaled_r65_1e8""",
}
TRIPLES = [(name, family, dtype_name) for (family, dtype_name), names in TABLE.items() for name in names.split()]

SEPARATED = ("diag", "tridiag", "blockdiag", "zero_line", "arrow", "graded3", "graded6", "scaled")
TIED = ("identity", "identity2", "twin", "wilkinson", "rank_one")
# the gradient is compared with autograd where a row's sign decides nothing: from 4 x 4 on (a 1 x 1 ... 3 x 3 matrix of these
# structures is negative definite on a quarter of the rows and more, which _check_backward's rule counts as a tie with the
# placeholder linear row: the cap of max(3, 0.05 B) kinks cannot hold there)
NO_GRADIENT_CHECK = ("diag_r1", "diag_r2", "diag_r3", "tridiag_r2", "tridiag_r3", "arrow_r2", "arrow_r3", "blockdiag_3_2")


def structure(name):
    return "rank_one" if name.startswith("rank_one") else ("zero_line" if name.startswith("zero_line") else name.split("_")[0])


BACKWARD_SEPARATED = [t for t in TRIPLES if structure(t[0]) in SEPARATED and t[0] not in NO_GRADIENT_CHECK]
BACKWARD_TIED = [t for t in TRIPLES if structure(t[0]) in TIED]


class Case:
    def __init__(self, name):
        builder, kwargs = CASES[name]
        self.name, self.structure = name, structure(name)
        self.raw = builder(**kwargs)
        self.k = len(self.raw["F"]) - 1
        self.r = self.raw["F"][0].shape[0]
        self.B = 64 if self.r <= 66 else 16
        self.x = rows(self.k, self.B, seed=sum(map(ord, name)))
        self.x.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def rows(k, B, seed):
    """``[B, k]`` fp64 holding fp32 numbers (module docstring)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.0, 2.0, size=(B, k))
    x[:2] *= 1e-4
    x[2] = 0.0
    for a in range(k):
        x[3 + 2 * a], x[4 + 2 * a] = 0.0, 0.0
        x[3 + 2 * a, a], x[4 + 2 * a, a] = 1.0, -1.0
    return x.astype(np.float32).astype(np.float64)


def build(raw, dtype=torch.float64):
    """``workloads.build_constraints`` under the default dtype the module will have (tests/test_gpu_lmi_wave.py::_layer)."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return workloads.build_constraints(raw)
    finally:
        torch.set_default_dtype(prev)


def evaluate(cs, x, dtype=torch.float64, grad=False):
    """The oracle on rows ``x [B, k]`` in ``dtype``: ``y [B, k]``, ``terms`` (every candidate of kappa for the unit
    direction; the last two columns are the two largest eigenvalues) and ``kappa`` of the row itself (``kappa(v / |v|) |v|``).
    ``grad``: also the tensors ``(x, y)`` autograd runs through."""
    buf = oracle.precompute(csd_from_cs(cs), dtype)
    xt = torch.from_numpy(np.array(x)).to(dtype).unsqueeze(2).requires_grad_(grad)
    yt = oracle.forward(buf, xt)
    unit = torch.nn.functional.normalize(xt.detach(), dim=1)
    terms = oracle.compute_kappa(buf, unit, terms=True).double().numpy()
    norm = np.linalg.norm(np.asarray(x, dtype=np.float64), axis=1)
    kappa = oracle.compute_kappa(buf, unit).double().numpy()[:, 0, 0] * norm
    out = dict(y=yt.detach().double().numpy()[:, :, 0], terms=terms, kappa=kappa, norm=norm)
    if grad:
        out["xt"], out["yt"] = xt, yt
    return out


@functools.lru_cache(maxsize=None)
def truth(name):
    """``(cs, fp64 evaluation)`` of a case, computed once and left unchanged."""
    c = case(name)
    cs = build(c.raw)
    ev = evaluate(cs, c.x)
    for val in ev.values():
        val.setflags(write=False)
    return cs, ev


@functools.lru_cache(maxsize=None)
def lapack32_error(name):
    """Per-row error of the reference's own fp32 arithmetic (LAPACK's fp32 eigvalsh) against the fp64 truth."""
    from helpers import rel_err_rows
    cs, ev = truth(name)
    y32 = evaluate(cs, case(name).x, torch.float32)["y"]
    return rel_err_rows(y32, ev["y"])


def lam_gap(terms):
    return np.abs(terms[:, -1] - terms[:, -2]) / np.maximum(np.abs(terms[:, -1]), 1e-30)


def kinks(terms, kappa, dtype_name):
    """The rows tests/test_gpu_lmi_wave.py::_check_backward sets aside: the two largest eigenvalues (nearly) tie, kappa
    within 1e-4 of 1, or the LMI level with the linear rows' maximum."""
    kink = (lam_gap(terms) < GAP[dtype_name]) | (np.abs(kappa - 1.0) < 1e-4)
    if terms.shape[1] > 2:
        top_lin = terms[:, :-2].max(axis=1)
        kink |= np.abs(top_lin - np.maximum(terms[:, -1], 0.0)) < 1e-4 * np.maximum(np.abs(top_lin), 1e-30)
    return kink


def spectrum(raw, x):
    """Eigenvalues ``[B, r]`` (ascending) of ``S(v) = -sum_a v_a F_a`` for the rows themselves (not their unit
    directions), numpy fp64."""
    F = np.stack(raw["F"][:-1], axis=0)
    return np.linalg.eigvalsh(-np.einsum("ba,aij->bij", np.asarray(x, dtype=np.float64), F))


# ---------------------------------------------------------------------------------------------------------------------
# soft cost (rayen_cost_lmi.hip shares lw::tridiagonalise and takes lambda_min(F(y))): sets beside cost_lmi_cases.SETS, on
# the plain rows above, held to cost_lmi_cases.check
# ---------------------------------------------------------------------------------------------------------------------
COST_SETS = {
    "diag_r8": ("diag_r8", ("float32", "float64")),
    "blockdiag_19_14": ("blockdiag_19_14", ("float64",)),
    "twin_r8_1e-4": ("twin_r8_1e-4", ("float32",)),
    "twin_r8_7e-9": ("twin_r8_7e-9", ("float64",)),
}
COST_TRIPLES = [(name, d) for name, (_, dtypes) in COST_SETS.items() for d in dtypes]


class CostCase(cost_lmi_cases.Case):
    """What ``cost_lmi_cases.check`` reads of a case, for a structured set on the rows of :func:`rows`."""

    def __init__(self, name):
        c = case(COST_SETS[name][0])
        self.name, self.B, self.k, self.r = name, c.B, c.k, c.r
        self.cs = build(c.raw)
        self.arrays = set_arrays(self.cs)
        self.y = c.x
        self.ref = cost_lmi_cases.reference(self.arrays, self.y)
        self.finite = ~np.isnan(self.ref["cost"])
        self.degenerate = np.zeros(self.B, dtype=bool)
        self.kept = self.finite & (self.ref["lmi"]["gap"] >= 1e-2)          # cost_lmi_cases' only exclusion
        self.fnorm = np.array([np.linalg.norm(Fa, 2) for Fa in self.arrays["F"][:-1]])


@functools.lru_cache(maxsize=None)
def cost_case(name):
    return CostCase(name)
