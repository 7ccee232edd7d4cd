"""fp64 reference of the soft cost / violation (rayen_amd/soft_cost.py, rayen_amd/csrc/rayen_cost.hip), written out one
constraint at a time like ``_one_by_one`` of tests/test_cost_computer.py, with the error bars of a working precision ``u``.

Per sample the reference returns ``cost``, ``worst``, ``which``, ``grad`` and every value ``vals [B, n]`` in the stacked order
``lin_ineq, quad, soc, lin_eq`` (the equality rows as ``|A2 y - b2|``), and for every value its condition scale ``S``: the sum
of the absolute values of all terms that are added to form it (the convention of tests/bar_reference.py; for a cone the norm
of the vector of such sums, plus the linear part's).

Bars (:func:`bounds`), for ANY summation order.  A value accumulated over a chain of depth ``d`` carries at most
``delta = (d + 8) u S``, with ``d = k`` (linear, equality), ``2 k`` (quadratic), ``k + rows`` (cone).  ``relu`` is
1-Lipschitz, so ``|D relu(g)^2| <= (2 relu(g) + delta) delta`` -- and exactly 0 where ``g < -delta`` (both sides answer 0);
the equalities carry ``(2 |e| + delta) delta``.  A gradient term ``2 relu(g) w`` carries ``2 (delta |w| + relu(g) delta_w +
delta delta_w)`` under the same gate, where ``delta_w`` is the error of the row's direction ``w``: ``u |a|`` (a stored row),
``(k + 8) u (|P||y| + |q|)`` (``P y + q``), and for a cone ``M'(u / n) - c`` with ``u = My + s``, ``n = ||u||``: the entries of
``u`` carry ``du = (k + 8) u (|M||y| + |s|)``, ``n`` carries ``dn = (k + rows + 8) u || |M||y| + |s| ||``, so ``u / n`` carries
``du / n + |u| dn / n^2`` (the ``delta / ||My + s||`` of the cone term), and the product with ``M'`` adds
``(rows + 8) u |M|'|u| / n``.  Finally ``grad`` is itself a sum of one term per stacked row: ``(rows_total + 8) u sum |term|``.
"""
import numpy as np


def reference(a, y):
    """``a``: ``rayen_amd.soft_cost.set_arrays(cs)``; ``y [B, k]`` fp64.  Returns a dict of per-sample arrays."""
    y = np.asarray(y, dtype=np.float64)
    B, k = y.shape
    ay = np.abs(y)
    vals, S, depth, dirs, ddirs_unit, kinds = [], [], [], [], [], []
    # dirs[j]: w [B, k] with d val_j / d y = w (for the |e| rows: of e);  ddirs_unit[j]: delta_w / u
    for arow, b in zip(a["A1"], a["b1"]):
        vals.append(y @ arow - b)
        S.append(ay @ np.abs(arow) + abs(b))
        depth.append(k)
        dirs.append(np.broadcast_to(arow, (B, k)))
        ddirs_unit.append(np.broadcast_to(np.abs(arow), (B, k)))
        kinds.append("ineq")
    for P, q, r in zip(a["P"], a["q"], a["r"]):
        Ps = 0.5 * (P + P.T)
        Py = y @ Ps
        vals.append(0.5 * np.sum(Py * y, axis=1) + y @ q + r)
        S.append(0.5 * np.sum((ay @ np.abs(Ps)) * ay, axis=1) + ay @ np.abs(q) + abs(r))
        depth.append(2 * k)
        dirs.append(Py + q)
        ddirs_unit.append((k + 8) * (ay @ np.abs(Ps) + np.abs(q)))
        kinds.append("ineq")
    at = 0
    soc_min_ratio = np.inf
    for j, rows in enumerate(a["soc_rows"]):
        M, s, c, d = a["M"][at:at + rows], a["s"][at:at + rows], a["c"][j], a["d"][j]
        at += rows
        u = y @ M.T + s
        su = ay @ np.abs(M).T + np.abs(s)
        n, sn = np.linalg.norm(u, axis=1), np.linalg.norm(su, axis=1)
        soc_min_ratio = min(soc_min_ratio, float(np.nanmin(n / sn)))
        vals.append(n - y @ c - d)
        S.append(sn + ay @ np.abs(c) + abs(d))
        depth.append(k + rows)
        safe = np.where(n > 0, n, 1.0)
        un = np.where((n > 0)[:, None], u / safe[:, None], 0.0)
        dirs.append(un @ M - c)
        dun = (k + 8) * su / safe[:, None] + np.abs(u) * ((k + rows + 8) * sn / safe ** 2)[:, None]
        ddirs_unit.append(dun @ np.abs(M) + (rows + 8) * (np.abs(un) @ np.abs(M)) + np.abs(c))
        kinds.append("ineq")
    for arow, b in zip(a["A2"], a["b2"]):
        vals.append(y @ arow - b)            # signed here; |.| below
        S.append(ay @ np.abs(arow) + abs(b))
        depth.append(k)
        dirs.append(np.broadcast_to(arow, (B, k)))
        ddirs_unit.append(np.broadcast_to(np.abs(arow), (B, k)))
        kinds.append("eq")
    signed = np.stack(vals, axis=1)
    S = np.stack(S, axis=1)
    is_eq = np.array([kd == "eq" for kd in kinds])
    act = np.where(is_eq[None, :], signed, np.where(signed < 0, 0.0, signed))        # relu that keeps a NaN | e
    cost = np.sum(act * act, axis=1)
    grad = np.zeros((B, k))
    for j in range(signed.shape[1]):
        grad += 2.0 * act[:, j:j + 1] * dirs[j]
    values = np.where(is_eq[None, :], np.abs(signed), signed)
    bad = np.isnan(cost)
    which = np.where(bad, -1, np.argmax(np.where(bad[:, None], 0.0, values), axis=1)).astype(np.int32)
    worst = np.where(bad, np.nan, np.max(np.where(bad[:, None], 0.0, values), axis=1))
    grad[bad] = np.nan
    return dict(cost=cost, worst=worst, which=which, grad=grad, vals=values, signed=signed, act=act, S=S,
                depth=np.asarray(depth), dirs=dirs, ddirs_unit=ddirs_unit, is_eq=is_eq, soc_min_ratio=soc_min_ratio)


def bounds(ref, u):
    """``(dvals [B, n], dcost [B], dgrad [B, k])`` at unit roundoff ``u`` (docstring of this module)."""
    delta = (ref["depth"][None, :] + 8) * u * ref["S"]
    act, signed, is_eq = np.abs(ref["act"]), ref["signed"], ref["is_eq"]
    gate = is_eq[None, :] | (signed > -delta)
    dcost = np.sum(np.where(gate, (2.0 * act + delta) * delta, 0.0), axis=1)
    n = signed.shape[1]
    dgrad = np.zeros_like(ref["grad"])
    terms = np.zeros_like(ref["grad"])
    for j in range(n):
        w, dw = np.abs(ref["dirs"][j]), u * ref["ddirs_unit"][j]
        dj, aj = delta[:, j:j + 1], act[:, j:j + 1]
        dgrad += np.where(gate[:, j:j + 1], 2.0 * (dj * w + aj * dw + dj * dw), 0.0)
        terms += 2.0 * aj * w
    dgrad += (n + 8) * u * terms
    return delta, dcost, dgrad


def which_is_decided(ref, dvals):
    """Rows where the two largest values differ by more than the sum of their bars (``which`` must match there)."""
    v = np.where(np.isnan(ref["vals"]), -np.inf, ref["vals"])
    if v.shape[1] < 2:
        return ~np.isnan(ref["cost"])
    order = np.argsort(-v, axis=1)
    rows = np.arange(v.shape[0])
    top, second = order[:, 0], order[:, 1]
    with np.errstate(invalid="ignore"):          # (a NaN row: every value is -inf here, and the row is not decided)
        gap = v[rows, top] - v[rows, second]
    # every other value is at most the second: its bar could be larger, so take the largest bar among the non-top values
    others = np.where(np.arange(v.shape[1])[None, :] == top[:, None], 0.0, dvals)
    return (gap > dvals[rows, top] + np.max(others, axis=1)) & ~np.isnan(ref["cost"])
