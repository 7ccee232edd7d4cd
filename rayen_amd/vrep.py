"""V-representation of ``{z : A z <= b}`` without cddlib: ``H_to_V(A, b) -> (V, R)``.

Same signature, return layout and conventions as the reference's ``rayen/utils.py::H_to_V`` (which calls pycddlib):
every column of ``V`` is a vertex, every column of ``R`` a ray, a lineality direction ``l`` appears as both ``l`` and
``-l`` (the reference's ``R = [R, -R[lin]]``), and an empty ``V`` or ``R`` is ``np.array([[]])`` (shape ``(1, 0)``).
The generator COUNTS equal cdd's -- degenerate vertices are merged, rays are extreme rays, a lineality space of
dimension d gives 2 d rays -- so a ``state_dict`` of the reference's ``method='Bar'`` layer (whose mapper is
``nv + nr`` wide) loads here.  Order and ray scaling differ from cdd's:

* vertices are sorted lexicographically by their coordinates;
* rays have unit length; the extreme rays of the pointed part come first, sorted lexicographically, followed by the
  lineality basis ``l_1 .. l_d`` and then ``-l_1 .. -l_d``.

Route: split off the lineality space ``null(A)``; the pointed part ``P'`` (coordinates in the row space of ``A``) is
homogenised into the cone ``{(w, t) : A' w - b t <= 0, t >= 0}``, which is cut by a hyperplane ``c.x = 1`` with ``c``
in the interior of the dual cone.  The slice is a bounded polytope whose vertices are the cone's extreme rays:
``t > 0`` gives the vertex ``w / t`` of ``P'``, ``t = 0`` an extreme ray ``w``.  Dimensions 0 and 1 have closed forms.
The slice's vertices are enumerated in one of two ways:

* when the upper-bound theorem (McMullen) caps its vertex count at ``max_generators`` or less, by
  ``scipy.spatial.HalfspaceIntersection`` around a Chebyshev centre found with HiGHS ``linprog``;
* otherwise -- many rows, which may be redundant or meet in few vertices (a box with redundant rows, a cross-polytope)
  -- by a walk over the vertex graph: start at an LP vertex, leave every vertex along its edges (the extreme rays of
  its local cone, from the same slicing at degenerate vertices), stop at the neighbouring vertex.  The walk's work
  grows with the vertices it finds, so it stops as soon as the count passes the cap.

The cap (65 536 generators by default) applies to the real generator count; beyond it ``TooManyGenerators`` is raised.
"""
from __future__ import annotations

import math
from collections import deque

import numpy as np
import scipy.linalg
import scipy.optimize
from scipy.spatial import HalfspaceIntersection, cKDTree

MAX_GENERATORS = 65536
_TOL = 1e-9          # feasibility / duplicate tolerance on the (unit-scale) slice
_ACTIVE = 1e-8       # a row is active at a slice vertex when its slack is at most this


class TooManyGenerators(ValueError):
    pass


def _rank_tol(s, shape):
    return max(shape) * np.finfo(float).eps * (s[0] if s.size else 0.0) * 1e3


def _upper_bound_vertices(m, d):
    """McMullen's upper-bound theorem: the most vertices a d-polytope with m facets can have."""
    if d <= 1:
        return 2
    if m <= d:
        return 1
    return math.comb(m - (d + 1) // 2, d // 2) + math.comb(m - d // 2 - 1, (d + 1) // 2 - 1)


def _dedupe(X, tol):
    """Columns of X with duplicates within ``tol`` (max-norm, relative to the scale) merged, in lexicographic order."""
    if X.shape[1] == 0:
        return X
    scale = max(1.0, float(np.max(np.abs(X))))
    X = np.where(np.abs(X) <= 1e-14 * scale, 0.0, X)          # (round-off zeros: a stable order)
    if X.shape[1] > 1:
        pairs = cKDTree(X.T).query_pairs(tol * scale, p=np.inf, output_type="ndarray")
        if len(pairs):
            keep = np.ones(X.shape[1], dtype=bool)
            keep[pairs.max(axis=1)] = False       # every cluster keeps its lowest index
            X = X[:, keep]
    return X[:, np.lexsort(X[::-1])]


def _too_many(count, cap):
    return TooManyGenerators(f"H_to_V: the set has {count} generators (vertices + rays), more than the cap of {cap}; "
                             "method='Bar' is not practical for it")


def _check_cap(count, cap):
    if count > cap:
        raise _too_many(count, cap)


def _cone_slice(G):
    """The cone {x : G x <= 0} (pointed) cut by c.x = 1: (c, U, Hs, hs) with the slice {c + U u : Hs u <= hs}."""
    Gn = G / np.linalg.norm(G, axis=1, keepdims=True)
    c = -Gn.sum(axis=0)                      # interior of the dual cone: c.x > 0 on the cone minus 0
    c /= np.linalg.norm(c)
    U = scipy.linalg.null_space(c[None, :])  # orthonormal basis of c's complement
    Hs, hs = Gn @ U, -(Gn @ c)
    keep = np.linalg.norm(Hs, axis=1) > 1e-12
    return c, U, Hs[keep], hs[keep]


def _interval(H, h):
    """Vertices of the bounded interval {u : H u <= h}, H a column."""
    a = H[:, 0]
    lo, hi = np.max(h[a < 0] / a[a < 0]), np.min(h[a > 0] / a[a > 0])
    return np.array([[lo, hi]]) if hi - lo > _TOL else np.array([[0.5 * (lo + hi)]])


def _qhull_vertices(H, h):
    """Vertices [d, count] of the bounded, full-dimensional polytope {u : H u <= h}, d >= 2, by qhull."""
    norms = np.linalg.norm(H, axis=1)
    d = H.shape[1]
    res = scipy.optimize.linprog(np.r_[np.zeros(d), -1.0], A_ub=np.c_[H, norms], b_ub=h,
                                 bounds=[(None, None)] * d + [(0, None)], method="highs")
    if res.status != 0 or res.x[-1] <= 1e-10:
        raise ValueError("H_to_V: the set has no interior (implicit equalities) or is empty")
    return _dedupe(HalfspaceIntersection(np.c_[H, -h], res.x[:d]).intersections.T, _TOL)


def _cone_rays(G):
    """Unit extreme rays [D, count] of the pointed cone {x : G x <= 0} in R^D (D >= 2), by qhull on its slice."""
    c, U, Hs, hs = _cone_slice(G)
    P = _interval(Hs, hs) if U.shape[1] == 1 else _qhull_vertices(Hs, hs)
    X = c[:, None] + U @ P
    return X / np.linalg.norm(X, axis=0, keepdims=True)


def _walk_vertices(H, h, cap):
    """Vertices [d, count] of the bounded polytope {u : H u <= h} by a walk over its vertex graph; raises
    ``TooManyGenerators`` as soon as more than ``cap`` vertices have been found."""
    d = H.shape[1]
    obj = np.arange(1, d + 1, dtype=np.float64) ** 0.5          # (a fixed, generic objective: the walk's start)
    res = scipy.optimize.linprog(obj, A_ub=H, b_ub=h, bounds=[(None, None)] * d, method="highs-ds")
    if res.status != 0:
        raise ValueError("H_to_V: the set is empty")

    def snap(x):
        act = h - H @ x <= _ACTIVE
        x = np.linalg.lstsq(H[act], h[act], rcond=None)[0] if act.sum() >= d else x
        return x, h - H @ x <= _ACTIVE

    def key(x):
        return tuple(np.round(x / 1e-7).astype(np.int64))

    x, act = snap(res.x)
    seen = {key(x): x}
    todo = deque([(x, act)])
    while todo:
        x, act = todo.popleft()
        Ha = H[act]
        if Ha.shape[0] == d:
            dirs = -np.linalg.inv(Ha)                            # simple vertex: the d edges
        else:
            dirs = _cone_rays(Ha)                                # degenerate vertex: the extreme rays of its cone
        slack = np.maximum(h - H @ x, 0.0)
        dirs = dirs / np.linalg.norm(dirs, axis=0, keepdims=True)
        Hd = H @ dirs                                            # [rows, edges]: every edge's ratio test at once
        with np.errstate(divide="ignore", invalid="ignore"):
            steps = np.where(Hd > 1e-12, slack[:, None] / Hd, np.inf).min(axis=0)
        for j in np.nonzero(np.isfinite(steps) & (steps > _TOL))[0]:
            y = x + steps[j] * dirs[:, j]
            if key(y) in seen:
                continue
            y, act_y = snap(y)
            k = key(y)
            if k not in seen:
                seen[k] = y
                if len(seen) > cap:
                    raise _too_many(f"more than {cap}", cap)
                todo.append((y, act_y))
    return _dedupe(np.array(list(seen.values())).T, _TOL)


def _pointed(Ap, b, cap):
    """Vertices [r, nv] and extreme rays [r, nr] of {w : Ap w <= b}, Ap of full column rank r."""
    m, r = Ap.shape
    if r == 0:
        if np.any(b < -1e-12):
            raise ValueError("H_to_V: the set is empty")
        return np.zeros((0, 1)), np.zeros((0, 0))
    if r == 1:
        a = Ap[:, 0]
        pos, neg = a > 0, a < 0
        hi = np.min(b[pos] / a[pos]) if pos.any() else None
        lo = np.max(b[neg] / a[neg]) if neg.any() else None
        if hi is not None and lo is not None and lo > hi + 1e-12 * max(1.0, abs(hi), abs(lo)):
            raise ValueError("H_to_V: the set is empty")
        verts = sorted({v for v in (lo, hi) if v is not None})
        if len(verts) == 2 and abs(verts[1] - verts[0]) <= 1e-12 * max(1.0, abs(verts[0]), abs(verts[1])):
            verts = verts[:1]
        rays = ([-1.0] if lo is None else []) + ([1.0] if hi is None else [])
        return np.array([verts], dtype=np.float64), np.array([rays], dtype=np.float64).reshape(1, len(rays))

    # the cone {x = (w, t) : G x <= 0}, G = [[Ap, -b], [0, -1]], pointed because Ap has full column rank
    G = np.zeros((m + 1, r + 1))
    G[:m, :r] = Ap
    G[:m, r] = -b
    G[m, r] = -1.0
    c, U, Hs, hs = _cone_slice(G)
    if _upper_bound_vertices(Hs.shape[0], r) <= cap:
        P = _qhull_vertices(Hs, hs)
    else:
        P = _walk_vertices(Hs, hs, cap)
    _check_cap(P.shape[1], cap)
    X = c[:, None] + U @ P                                      # [r+1, count], each on c.x = 1
    t = X[r]
    is_vertex = t > _TOL * np.max(np.abs(X), axis=0)
    verts = X[:r, is_vertex] / t[is_vertex]
    rays = X[:r, ~is_vertex]
    rays = rays / np.linalg.norm(rays, axis=0, keepdims=True) if rays.shape[1] else rays
    return _dedupe(verts, _TOL), _dedupe(rays, _TOL)


def H_to_V(A, b, max_generators=MAX_GENERATORS):
    """``(V, R)``: vertices and rays of ``{z : A z <= b}`` as columns (module docstring for the conventions).
    More than ``max_generators`` generators raise ``TooManyGenerators``."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    if A.ndim != 2 or A.shape[0] != b.shape[0]:
        raise ValueError(f"H_to_V: A {A.shape} and b {b.shape} do not match")
    n = A.shape[1]
    if n == 0:
        raise ValueError("H_to_V: the set has dimension 0")
    row_norm = np.linalg.norm(A, axis=1)
    zero = row_norm <= 1e-12 * max(1.0, float(row_norm.max(initial=0.0)))
    if np.any(b[zero] < -1e-12):
        raise ValueError("H_to_V: the set is empty (a row 0 z <= b with b < 0)")
    A, b = A[~zero], b[~zero]
    # row space (pointed part) and null space (lineality) of A
    if A.shape[0]:
        _, s, Vt = np.linalg.svd(A)
        rank = int(np.sum(s > _rank_tol(s, A.shape)))
    else:
        Vt, rank = np.eye(n), 0
    Q = Vt[:rank].T                      # [n, rank]
    L = Vt[rank:].T                      # [n, n - rank]
    if L.shape[1]:
        # a deterministic basis of the lineality space: reduced against the coordinate axes, unit columns
        L = scipy.linalg.orth(L @ L.T @ np.eye(n)[:, np.argsort(-np.linalg.norm(L, axis=1), kind="stable")])
        for j in range(L.shape[1]):
            i = int(np.argmax(np.abs(L[:, j]) > 1e-9))
            if L[i, j] < 0:
                L[:, j] = -L[:, j]
    _check_cap(2 * L.shape[1], max_generators)
    W, D = _pointed(A @ Q, b, max_generators - 2 * L.shape[1])
    V = Q @ W if rank else np.zeros((n, W.shape[1]))
    R = Q @ D if D.shape[1] else np.zeros((n, 0))
    R = np.concatenate([R, L, -L], axis=1)
    _check_cap(V.shape[1] + R.shape[1], max_generators)
    if R.size == 0:
        R = np.array([[]])
    if V.size == 0:
        V = np.array([[]])
    return V, R
