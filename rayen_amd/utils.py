"""Small host-side helpers that the constraint description and the layer share.

Mirrors the helper surface of the reference's ``rayen/utils.py`` that is on the
RAYEN path and that this package itself calls (``verify`` utils.py:21-23,
``getAllPqrFromQcs`` / ``getAllMscdFromSocs`` utils.py:25-46, the symmetry / non-zero
checks utils.py:113-121, ``all_equal`` utils.py:245-251).  Everything else in the
reference's utils (timers, pycddlib ``H_to_V``, power-iteration experiments,
pickle helpers) serves the harness or the paper baselines and is out of scope
(SURVEY.md §2 row 5).  ``rref`` and ``removeRedundantEquationsFromEqualitySystem``
(utils.py:138-207) are restated here for ``method='DC3'``.
"""
from __future__ import annotations

import numpy as np

_BOLD = "\033[1m"
_RESET = "\033[0m"
_COLOURS = {"blue": "\033[34m", "green": "\033[32m"}


def _print_bold(colour: str, text: str) -> None:
    print(f"{_BOLD}{_COLOURS[colour]}{text}{_RESET}")


def printInBoldBlue(data_string):
    _print_bold("blue", data_string)


def printInBoldGreen(data_string):
    _print_bold("green", data_string)


def verify(condition, message="Condition not satisfied"):
    """Raise ``RuntimeError(message)`` when ``condition`` is false (utils.py:21-23)."""
    if not bool(condition):
        raise RuntimeError(message)


def getAllPqrFromQcs(qcs):
    """Split a list of quadratic constraints into three parallel lists (utils.py:25-33)."""
    return [qc.P for qc in qcs], [qc.q for qc in qcs], [qc.r for qc in qcs]


def getAllMscdFromSocs(socs):
    """Split a list of SOC constraints into four parallel lists (utils.py:35-46)."""
    return ([soc.M for soc in socs], [soc.s for soc in socs],
            [soc.c for soc in socs], [soc.d for soc in socs])


def isZero(A):
    return not np.any(A)


def checkMatrixisNotZero(A):
    verify(not isZero(A))


def checkMatrixisSymmetric(A):
    verify(A.shape[0] == A.shape[1])
    verify(np.allclose(A, A.T))


def all_equal(iterator):
    items = list(iterator)
    return all(item == items[0] for item in items[1:])


def rref(B, tol=1e-8):
    """Reduced row echelon form by Gauss-Jordan elimination with partial pivoting (utils.py:138-179).

    Returns ``(R, pivots_pos, row_exchanges)``: ``pivots_pos`` lists ``(row, column)`` of every pivot, ``row_exchanges``
    the permutation of the input's rows.  A column whose largest remaining entry is at most ``tol`` holds no pivot and
    its remaining entries are set to zero.  Same pivot choice as the reference (first largest magnitude at or below the
    current row), so the same columns become the dependent variables of DC3's completion."""
    R = np.array(B, dtype=np.float64, copy=True)
    rows, cols = R.shape
    pivots_pos = []
    row_exchanges = np.arange(rows)
    r = 0
    for c in range(cols):
        if r == rows:
            break
        pivot = r + int(np.argmax(np.abs(R[r:, c])))
        if np.abs(R[pivot, c]) <= tol:
            R[r:, c] = 0.0
            continue
        pivots_pos.append((r, c))
        if pivot != r:
            R[[r, pivot], c:] = R[[pivot, r], c:]
            row_exchanges[[r, pivot]] = row_exchanges[[pivot, r]]
        R[r, c:] = R[r, c:] / R[r, c]
        lead = R[r, c:].copy()
        for i in range(rows):
            if i != r:
                R[i, c:] = R[i, c:] - R[i, c] * lead
        r += 1
    return R, pivots_pos, row_exchanges


def removeRedundantEquationsFromEqualitySystem(A, b):
    """``(A', b')`` with the fewest rows such that ``A' x = b'`` has the solutions of ``A x = b``: the non-zero rows of
    the rref of ``[A | b]`` (utils.py:184-207)."""
    Ab, _, _ = rref(np.concatenate((A, b), axis=1))
    Ab = Ab[np.linalg.norm(Ab, axis=1) >= 1e-7, :]
    if Ab.shape[0] > 0:
        assert np.linalg.matrix_rank(Ab) == Ab.shape[0]
    return Ab[:, :-1].reshape((-1, A.shape[1])), Ab[:, -1].reshape((-1, 1))
