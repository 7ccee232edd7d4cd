"""The crafted block plans of the wide kernels' sweep (tests/test_wide_sweep_host.py, tests/test_gpu_wide_sweep.py): real
geometry (``workloads.random_lin_quad_soc`` through ``ConstraintModule.packed_constants``), the rows of ``W`` moved.

``relayout`` returns a pack whose ``W`` holds the same rows at chosen places: a segment's aux row(s) away from its rows,
rows that belong to no segment in between (filled with ``POISON``), a linear run cut in two, exact copies of linear rows.
The truth of every case is fp64 on the RELAID pack: ``packed_eval.evaluate`` for y / kappa / active, fp64 autograd through
``rayen_amd.eager.PackedEvaluator`` for grad_v (``truth``); tests/test_wide_sweep_host.py first holds the relaid pack's fp64
outputs to the packer's own layout at 1e-12.

Inputs of every case: ``wide_fused_cases.inputs(n, 97)`` (rows 0-3 interior, 4-7 far outside, row 8 zero) with rows 9
onward multiplied by the case's ``scale``; upstream gradients uniform in [-1, 1] (seed 177).

Counts of the final recipes (``coverage(name)``; tests/test_wide_sweep_host.py holds them to the conditions of the table in
DESIGN.md, "Wide kernels: the sweep"; clipped: kappa64 > 1; active by type among the clipped rows; kink rows: the two
largest fp64 candidates of different constraints within 1e-4 relative, or |kappa64 - 1| <= 1e-4):

    case          n    k    rows  nb_w  clipped    LIN / SYM / FAC / SOC active  kink rows  what the plan is
    nbw2          129  129    57    2   48 of 97   48 /  0 /  0 /  0             0          LIN rows 7..56: waves 1 and 3 (0 and 2 own nothing)
    nbw3          129  129    87    3   49 of 97   49 /  0 /  0 /  0             0          LIN rows 7..86: waves 1, 2, 3 (0 owns nothing)
    nbw5          129  129   147    5   49 of 97   49 /  0 /  0 /  0             0          LIN rows 7..146: waves 0-3, wave 3 two blocks
    nbw7          129  129   207    7   50 of 97   50 /  0 /  0 /  0             0          LIN rows 7..206: waves 0-3 with 1 / 2 / 2 / 2 blocks
    fac_edges     135  135   131    5   42 of 97   20 /  0 / 22 /  0             0          QUAD_FAC of 33 / 1 / 31 / 32 rows from rows 31 / 65 / 67 / 99, active on 4 / 9 / 3 / 6
    aux_far       136  136   226    8   46 of 97    1 / 24 / 16 /  5             0          aux rows 192..195 (block 6, wave 3); the rows of SYM, FAC, SOC in blocks 0-4 (waves 0-2)
    soc_straddle  161  161   157    5   45 of 97    7 /  0 / 15 / 23             0          a cone's aux rows 31 | 32 (waves 0 | 1), that cone active on 12
    gaps          200  200   333   11   44 of 97    1 / 24 / 17 /  2             0          44 rows of nobody, one or more in every block that one segment does not fill
    lin_ties      129  129   160    5   47 of 97   47 /  0 /  0 /  0             0          copies at rows (40, 45), (104, 142), (7, 76): the maximiser on 15 / 11 / 10 inputs
    lin_ties_cut  129  129   160    5   47 of 97   47 /  0 /  0 /  0             0          the same, the run cut at row 70: pair (7, 76) lies across two segments
    eq_k161       160  161    40    2   49 of 97   49 /  0 /  0 /  0             0          NA_E != I, k % 32 = 1, no non-linear segment
    eq_k191       160  191    83    3   46 of 97   23 /  0 /  0 / 23             0          k % 32 = 31, one non-linear segment (workspace 0: no grouping)
    eq_k192       160  192   535   17   48 of 97    2 / 30 /  7 /  9             0          k % 32 = 0, seven non-linear segments
    nl5           136  136   307   10   54 of 97    3 / 12 / 24 / 15             0          five non-linear segments active on 12 / 21 / 3 / 6 / 9; two tiles with 5 of them

``lin_ties_plain`` is the set of ``lin_ties`` in the packer's layout (no copy), for the bit comparison of kappa.  A low-rank
``P = w 2 C'C`` with C of r rows packs as a QUAD_FAC segment of r + 1 rows (the gradient at y0 adds a direction): the one-row
segment of ``fac_edges`` has P = 0.
"""
import functools

import numpy as np
import torch

import wide_fused_bwd_cases as WB
import wide_fused_cases as F
from rayen_amd import _lib, workloads
from rayen_amd.pack import PackedConstants, Segment

B = 97
POISON = 1e30            # rows of W that belong to no segment
KINK_GAP = 1e-4          # tests/test_gpu_backward.py::KINK_GAP[torch.float32]
_NONLINEAR = (_lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC, _lib.SEG_SOC)


def naux(seg_type):
    return 1 if seg_type in (_lib.SEG_QUAD_SYM, _lib.SEG_QUAD_FAC) else 2 if seg_type == _lib.SEG_SOC else 0


# ---------------------------------------------------------------- moving the rows
def relayout(consts, order=None, gaps=None, aux_after=None, split_lin=None, dup_lin=None, poison=POISON):
    """A pack with the rows of ``consts`` at other places of ``W``; ``row0`` / ``aux_row`` follow.

    Segment indices below are those of the table AFTER ``split_lin``, which is the table of the result:

    ``split_lin``  (s, at): the linear segment s becomes two, rows [0, at) as segment s and [at, nrows) as segment s + 1
    ``dup_lin``    [(s, src, at), ...]: an exact copy of row ``src`` of the linear segment s is inserted so that it sits at
                   place ``at > src`` of the segment (applied in the order given: later entries see the earlier copies)
    ``order``      the segments in the order their rows are laid (default: table order); a segment's aux row(s) lie
                   directly before its rows unless ``aux_after`` moves them
    ``aux_after``  {s: t}: the aux row(s) of s lie directly behind the rows of segment t (t = s: behind its own rows;
                   t = None: behind everything laid by ``order``), several behind the same t in rising s
    ``gaps``       {key: count}: rows of no segment, every element ``poison``; key ('before', s): before the aux row(s) (or
                   the rows, where the aux rows were moved) of s, ('aux', s): between the aux row(s) and the rows of s,
                   ('after', s): behind the rows of s (before aux rows moved there), ('tail', s): behind the aux rows moved
                   behind s, 'end': behind everything (before aux rows moved to the end), 'tail': the very last rows

    The result carries ``origin``: for every segment the index of the segment of ``consts`` it came from, and ``gap_rows``."""
    gaps, aux_after = dict(gaps or {}), dict(aux_after or {})
    n = consts.n
    W = np.asarray(consts.W, dtype=np.float64)
    parts = []                          # [type, rows, aux rows, f0, f1, origin]
    for i, s in enumerate(consts.segments):
        assert s.type != _lib.SEG_LMI
        a = W[s.aux_row:s.aux_row + naux(s.type)] if naux(s.type) else np.zeros((0, n))
        parts.append([s.type, W[s.row0:s.row0 + s.nrows].copy(), a.copy(), s.f0, s.f1, i])
    if split_lin is not None:
        s, at = split_lin
        t, rows, a, f0, f1, origin = parts[s]
        assert t == _lib.SEG_LIN and 0 < at < rows.shape[0]
        parts[s:s + 1] = [[t, rows[:at].copy(), a, f0, f1, origin], [t, rows[at:].copy(), a, f0, f1, origin]]
    for s, src, at in (dup_lin or []):
        assert parts[s][0] == _lib.SEG_LIN and 0 <= src < at <= parts[s][1].shape[0]
        parts[s][1] = np.insert(parts[s][1], at, parts[s][1][src], axis=0)
    order = list(range(len(parts))) if order is None else list(order)
    assert sorted(order) == list(range(len(parts)))
    assert all(naux(parts[s][0]) for s in aux_after)
    blocks, row0, aux_row, gap_rows = [], {}, {}, []
    count = [0]

    def lay(block):
        at = count[0]
        blocks.append(block)
        count[0] += block.shape[0]
        return at

    def gap(key):
        c = gaps.pop(key, 0)
        if c:
            at = lay(np.full((c, n), float(poison)))
            gap_rows.extend(range(at, at + c))

    def moved_behind(t):
        for s in sorted(x for x in aux_after if aux_after[x] == t):
            aux_row[s] = lay(parts[s][2])

    for s in order:
        gap(("before", s))
        if naux(parts[s][0]) and s not in aux_after:
            aux_row[s] = lay(parts[s][2])
        gap(("aux", s))
        row0[s] = lay(parts[s][1])
        gap(("after", s))
        moved_behind(s)
        gap(("tail", s))
    gap("end")
    moved_behind(None)
    gap("tail")
    assert not gaps, f"gap keys that name nothing: {sorted(map(str, gaps))}"
    segments = [Segment(t, row0[s], rows.shape[0], aux_row=aux_row.get(s, -1), f0=f0, f1=f1)
                for s, (t, rows, a, f0, f1, origin) in enumerate(parts)]
    out = PackedConstants(k=consts.k, n=n, W=np.ascontiguousarray(np.concatenate(blocks, axis=0)), segments=segments,
                          NA_E=consts.NA_E, y0=consts.y0, out_identity=consts.out_identity,
                          dropped_segments=consts.dropped_segments)
    out.origin = [p[5] for p in parts]
    out.gap_rows = gap_rows
    return out


def zero_gaps(consts):
    """The same pack with the rows of no segment zero."""
    W = consts.W.copy()
    W[consts.gap_rows] = 0.0
    out = PackedConstants(k=consts.k, n=consts.n, W=W, segments=list(consts.segments), NA_E=consts.NA_E, y0=consts.y0,
                          out_identity=consts.out_identity, dropped_segments=consts.dropped_segments)
    out.origin, out.gap_rows = list(consts.origin), list(consts.gap_rows)
    return out


# ---------------------------------------------------------------- the sets
NBW = {"nbw2": 50, "nbw3": 80, "nbw5": 140, "nbw7": 200}                    # linear rows
EQ_K = {"eq_k161": 161, "eq_k191": 191, "eq_k192": 192}
CASES = (*NBW, "fac_edges", "aux_far", "soc_straddle", "gaps", "lin_ties", "lin_ties_cut", *EQ_K, "nl5")
FAC_ROWS = (33, 1, 31, 32)              # fac_edges: rows of the four QUAD_FAC segments, in the order laid
# (quadratics, cones): how far each is shrunk about y0 (``_tighten``), tuned on the host until every segment has its share
TIGHTEN = {"fac_edges": ((3.5, 2.0, 3.4, 2.9), ()), "aux_far": ((14.0, 11.0), (4.0,)), "soc_straddle": ((6.0,), (2.6, 2.6)),
           "gaps": ((15.0, 5.5), (2.1,)), "eq_k191": ((), (2.0,)), "eq_k192": ((9.0, 13.0, 12.0, 1.3), (2.8, 2.8, 2.8)),
           "nl5": ((15.0, 5.0, 1.3), (3.0, 3.6))}
# lin_ties: the copied rows (rows of the packer's run that are the fp64 maximiser on ten or more of the 97 inputs each) and
# where their copies are inserted, placements (i), (ii), (iii); with all three in, the pairs sit at rows (40, 45) -- the
# first in the lower half-wave's rows of block 1, its copy in the upper one's --, (104, 142) and (7, 76) of the run
TIE_ROWS = (40, 102, 7)
TIE_AT = (45, 140, 75)
TIE_CUT = 70
SCALE = {"nbw2": 0.035, "nbw3": 0.026, "nbw5": 0.02, "nbw7": 0.02, "fac_edges": 0.026, "aux_far": 0.013, "soc_straddle": 0.019,
         "gaps": 0.014, "lin_ties": 0.023, "lin_ties_cut": 0.023, "eq_k161": 0.036, "eq_k191": 0.03, "eq_k192": 0.013,
         "nl5": 0.016}


def _low_rank(r, k, rng, rank, w):
    """``P = w 2 C'C`` with C of ``rank`` rows: the packer stores it as a QUAD_FAC segment of ``rank + 1`` rows (the gradient
    at y0 adds one direction to the form)."""
    Cm = rng.uniform(-1.0, 1.0, size=(rank, k))
    r["P"].append(w * 2.0 * Cm.T @ Cm)
    r["q"].append(rng.uniform(-1.0, 1.0, size=(k, 1)))
    r["r"].append(rng.uniform(-1.0, -0.1, size=(1, 1)))


def _tighten(r, quads=(), socs=()):
    """Shrinks quadratic i / cone j about y0 = 0 by the factor given (its candidate of kappa grows by exactly that factor):
    the knob with which every segment gets its share of the inputs."""
    for i, c in enumerate(quads):
        r["P"][i], r["q"][i] = r["P"][i] * c * c, r["q"][i] * c
    for j, c in enumerate(socs):
        r["M"][j], r["c"][j] = r["M"][j] * c, r["c"][j] * c
    return r


@functools.lru_cache(maxsize=None)
def raw(name):
    return _tighten(_raw(name), *TIGHTEN.get(name, ((), ())))


def _raw(name):
    if name in NBW:
        return workloads.random_lin_quad_soc(k=129, m=NBW[name], n_quad=0, n_soc=1, r_M=5, seed=300 + NBW[name])
    if name == "fac_edges":
        r = workloads.random_lin_quad_soc(k=135, m=20, n_quad=0, n_soc=0, seed=311)
        rng = np.random.default_rng(1311)
        for rows in FAC_ROWS:
            _low_rank(r, 135, rng, rows - 1, 0.1)
        return r
    if name == "aux_far":
        r = workloads.random_lin_quad_soc(k=136, m=30, n_quad=1, n_soc=1, r_M=20, seed=312)
        r["P"] = [0.002 * P for P in r["P"]]
        _low_rank(r, 136, np.random.default_rng(1312), 3, 0.1)
        return r
    if name == "soc_straddle":
        r = workloads.random_lin_quad_soc(k=161, m=40, n_quad=0, n_soc=2, r_M=41, seed=313)
        _low_rank(r, 161, np.random.default_rng(1313), 10, 0.1)
        return r
    if name == "gaps":
        r = workloads.random_lin_quad_soc(k=200, m=40, n_quad=1, n_soc=1, r_M=41, seed=314)
        r["P"] = [0.002 * P for P in r["P"]]
        _low_rank(r, 200, np.random.default_rng(1314), 3, 0.1)
        return r
    if name in ("lin_ties", "lin_ties_cut", "lin_ties_plain"):
        return workloads.random_lin_quad_soc(k=129, m=150, n_quad=0, n_soc=1, r_M=5, seed=315)
    if name in EQ_K:
        k = EQ_K[name]
        if name == "eq_k161":
            r = workloads.random_lin_quad_soc(k=k, m=40, n_quad=0, n_soc=0, seed=316)
        elif name == "eq_k191":
            r = workloads.random_lin_quad_soc(k=k, m=40, n_quad=0, n_soc=1, r_M=41, seed=317)
        else:
            r = workloads.random_lin_quad_soc(k=k, m=40, n_quad=2, n_soc=3, r_M=41, seed=318)
            r["P"] = [0.002 * P for P in r["P"]]
            rng = np.random.default_rng(1318)
            _low_rank(r, k, rng, 3, 0.1)
            _low_rank(r, k, rng, 37, 0.5)
        r["A2"] = np.random.default_rng(2316 + k).uniform(-1, 1, (k - 160, k))
        r["b2"] = np.zeros((k - 160, 1))
        return r
    if name == "nl5":
        r = workloads.random_lin_quad_soc(k=136, m=40, n_quad=1, n_soc=2, r_M=41, seed=319)
        r["P"] = [0.002 * P for P in r["P"]]
        rng = np.random.default_rng(1319)
        _low_rank(r, 136, rng, 3, 0.1)
        _low_rank(r, 136, rng, 37, 0.5)
        return r
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def cs(name):
    return workloads.build_constraints(raw(name))


@functools.lru_cache(maxsize=None)
def packed(name):
    """The packer's own layout of a case's set."""
    from rayen_amd.constraint_module import ConstraintModule
    return ConstraintModule(cs(name), create_map=False).packed_constants()


def _by_type(p, t):
    return [i for i, s in enumerate(p.segments) if s.type == t]


@functools.lru_cache(maxsize=None)
def consts(name):
    """The relaid pack of a case."""
    p = packed(name)
    if name in NBW:
        return relayout(p, order=[1, 0])                         # the cone's 7 rows, then the linear run from row 7
    if name == "fac_edges":
        fac = _by_type(p, _lib.SEG_QUAD_FAC)
        assert [p.segments[i].nrows for i in fac] == list(FAC_ROWS)
        return relayout(p, gaps={("after", 0): 10})              # 20 linear rows, 10 of nobody, aux 30, rows 31..63, ...
    if name == "aux_far":
        (sym,), (fac,), (soc,) = (_by_type(p, t) for t in _NONLINEAR)
        return relayout(p, order=[sym, fac, soc, 0], aux_after={sym: soc, fac: soc, soc: soc},
                        gaps={("after", soc): 192 - (136 + p.segments[fac].nrows + 20)})
    if name == "soc_straddle":
        (fac,), (soc_a, soc_b) = _by_type(p, _lib.SEG_QUAD_FAC), _by_type(p, _lib.SEG_SOC)
        return relayout(p, order=[fac, soc_a, soc_b, 0], gaps={("after", fac): 31 - (1 + p.segments[fac].nrows)})
    if name == "gaps":
        (sym,), (fac,), (soc,) = (_by_type(p, t) for t in _NONLINEAR)
        # block 0: a poisoned row, 30 linear rows from row 1, a poisoned row; block 1: the other 10 linear rows as a second
        # segment between poisoned rows, the quadratic's aux row, a poisoned row, its 200 rows from row 47; ...
        return relayout(p, split_lin=(0, 30), order=[0, 1, sym + 1, fac + 1, soc + 1],
                        gaps={("before", 0): 1, ("after", 0): 1, ("before", 1): 1, ("after", 1): 2, ("aux", sym + 1): 1,
                              ("after", sym + 1): 3, ("aux", fac + 1): 2, ("after", fac + 1): 1, ("before", soc + 1): 20,
                              ("aux", soc + 1): 9, ("after", soc + 1): 2, "tail": 1})
    if name in ("lin_ties", "lin_ties_cut"):
        # (the copy that lands last goes in first: the places of the earlier rows do not move under it)
        dups = [(0, src, at) for src, at in sorted(zip(TIE_ROWS, TIE_AT), key=lambda x: -x[1])]
        if name == "lin_ties":
            return relayout(p, dup_lin=dups)
        # the copies, then the cut: pair (i) and the first row of pair (iii) in segment 0, its copy and pair (ii) in segment 1
        return relayout(relayout(p, dup_lin=dups), split_lin=(0, TIE_CUT))
    return relayout(p)                                           # eq_k*, nl5, lin_ties_plain: the packer's layout


def inputs(name):
    """``[97, n, 1]`` fp32."""
    x = F.inputs(packed(name).n, B)
    x[9:] *= SCALE[name.replace("_plain", "")]
    return x


def grads(name):
    gen = torch.Generator().manual_seed(177)
    return torch.empty(B, packed(name).k, dtype=torch.float32).uniform_(-1, 1, generator=gen)


# ---------------------------------------------------------------- the truth, fp64 on the host
def _as_pack(c):
    return c if isinstance(c, PackedConstants) else consts(c)


def evaluate64(c, v):
    import packed_eval
    return packed_eval.evaluate(_as_pack(c), v)


def truth_grad(c, v, G):
    """fp64 autograd through ``PackedEvaluator`` on the pack; a zero row has kappa = 0 on a neighbourhood, so its gradient is
    ``NA_E' g`` (autograd divides 0 by 0 in the square roots there)."""
    from rayen_amd.eager import PackedEvaluator
    c = _as_pack(c)
    ev = PackedEvaluator(c, torch.float64, "cpu")
    vt = torch.as_tensor(np.asarray(v, dtype=np.float64)).clone().requires_grad_(True)
    Gt = torch.as_tensor(np.asarray(G, dtype=np.float64))
    y, _ = ev.project(vt)
    (y * Gt).sum().backward()
    g = vt.grad.numpy().copy()
    zero = ~np.any(np.asarray(v) != 0, axis=1)
    g[zero] = np.asarray(G, dtype=np.float64)[zero] @ c.NA_E
    return g


@functools.lru_cache(maxsize=None)
def truth(name):
    """(y64, kappa64, active64, grad64) of a case on its relaid pack, computed once and left unchanged."""
    v = inputs(name)[:, :, 0].double().numpy()
    y, kappa, active = evaluate64(name, v)
    g = truth_grad(name, v, grads(name).double().numpy())
    for a in (y, kappa, active, g):
        a.setflags(write=False)
    return y, kappa, active, g


def constraint_values(c, v):
    """[B, constraints] fp64: every linear row (copies of a row folded into the first) and every non-linear segment."""
    c = _as_pack(c)
    cols, seen = [], {}
    for s, cand in zip(c.segments, WB.candidates64(c, v)):
        if s.type != _lib.SEG_LIN:
            cols.append(cand[:, 0])
            continue
        for j in range(s.nrows):
            key = c.W[s.row0 + j].tobytes()
            if key not in seen:
                seen[key] = True
                cols.append(cand[:, j])
    return np.stack(cols, axis=1)


def kink_rows(c, v):
    """Rows where the two largest candidates of different constraints lie within ``KINK_GAP`` relative, or kappa within 1e-4
    of 1."""
    vals = np.sort(constraint_values(c, v), axis=1)
    top, second = vals[:, -1], (vals[:, -2] if vals.shape[1] > 1 else np.zeros(len(vals)))
    kappa = np.maximum(top, 0.0)
    second = np.maximum(second, 0.0)
    tie = (kappa > 0) & (kappa - second <= KINK_GAP * kappa)
    return tie | (np.abs(kappa - 1.0) <= 1e-4)


@functools.lru_cache(maxsize=None)
def coverage(name):
    c = consts(name)
    v = inputs(name)[:, :, 0].double().numpy()
    kappa, seg = WB.active64(c, v)
    clipped = kappa > 1
    by_seg = {i: int(np.sum(clipped & (seg == i))) for i in range(len(c.segments))}
    by_type = {}
    for i, cnt in by_seg.items():
        by_type[c.segments[i].type] = by_type.get(c.segments[i].type, 0) + cnt
    keys = [len(set(int(s) for s, cl in zip(seg[t:t + 32], clipped[t:t + 32]) if cl and c.segments[s].type != _lib.SEG_LIN))
            for t in range(0, B, 32)]
    return dict(clipped=int(clipped.sum()), by_seg=by_seg, by_type=by_type, nl_keys_per_tile=keys,
                kinks=int(kink_rows(c, v).sum()))


# ---------------------------------------------------------------- the launchers' grids (also in the two *_cases modules)
def plans(c):
    """(forward plan, its segment plans, backward plan) of a pack."""
    c = _as_pack(c)
    fp, sp = F.plan(c.n, c.k, c.W.shape[0], int(c.out_identity), F.seg_inputs(c.segments))
    return fp, sp, WB.plan(c.n, c.k, int(c.out_identity), WB.widest_t(c.segments))


def second_round_batch(slots):
    """A batch whose tiles need three rounds of a grid of ``slots`` workgroups, the last tile partial."""
    return 32 * (2 * slots + slots // 2) + 13
