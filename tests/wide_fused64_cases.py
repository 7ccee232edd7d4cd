"""The sets and inputs of the fp64 fused wide forward's tests (tests/test_wide_fused64_host.py,
tests/test_gpu_wide_fused64.py), and a Python restatement of the block plan in rayen_amd/csrc/rayen_wide_fused64_layout.h.

    case            what it exercises
    n65             one past the threshold (ops._WIDE_MIN_N[float64]); K tail of one group (kp = 72: two chunks of four
                    groups and one more); 17 linear rows, a quadratic of 65 rows and a cone of 17: each one row past a block
    n66_one_row     a single row: three waves own nothing
    k190_n160       (wide_fused_cases) NA_E != I; k % 16 = 14; y used as scratch
    s32_last        the largest n whose plan picks 32 samples, found from the restated plan (``s32_last_n``)
    s16_first       the next n: 16 samples
    k1024           (wide_fused_cases) the envelope's last n
    k1025           (wide_fused_cases) one past it: the refusal
    plan_a          relaid: a cone's aux rows at rows 15 | 16, blocks 0 | 1, waves 0 | 1
    plan_b2/3/5/7   relaid: nb_w of 2, 3, 5 and 7 blocks of 16 (a cone's 7 rows, then the linear run from row 7)
    plan_c          relaid: QUAD_FAC segments of 17 / 1 / 15 / 16 rows (the one-row segment has P = 0)
    plan_d          (wide_sweep_cases "gaps") rows of no segment, POISON, in every block that one segment does not fill
    plan_e          (wide_sweep_cases "lin_ties" / "lin_ties_cut" / "lin_ties_plain") exact copies of a linear row inside a
                    block, across blocks and across a segment cut

Inputs of every case: ``wide_fused_cases.inputs(n, B)`` as doubles (rows 0-3 interior, 4-7 far outside, row 8 zero), rows 9
onward multiplied by ``SCALE`` (so that a fair share of them is not clipped); the sets taken from wide_sweep_cases keep
that module's inputs."""
import functools

import numpy as np

import wide_fused_cases as F
import wide_sweep_cases as WS
from rayen_amd import _lib, workloads

OWN = ("n65", "n66_one_row", "k190_n160", "s32_last", "s16_first", "k1024")
PLAN_B = {"plan_b2": 20, "plan_b3": 35, "plan_b5": 70, "plan_b7": 100}          # linear rows
RELAID = ("plan_a", *PLAN_B, "plan_c", "plan_d", "plan_e", "plan_e_cut")
CASES = (*OWN, *RELAID)
FAC_ROWS = (17, 1, 15, 16)
SCALE = 0.03
B = 97
_FROM_SWEEP = {"plan_d": "gaps", "plan_e": "lin_ties", "plan_e_cut": "lin_ties_cut", "plan_e_plain": "lin_ties_plain"}

# ---------------------------------------------------------------- the block plan, restated
BLOCK, WAVES, MAX_N, LDS = 16, 4, 1024, 160 * 1024 - 256
block_start, wave_of, seg_inputs = F.block_start, F.wave_of, F.seg_inputs


def _scratch(nb_w, S, segs):
    words, seg_plans = 0, []
    for row0, nrows, slots, naux in segs:
        first = row0 // BLOCK if nrows > 0 else 0
        last = (row0 + nrows - 1) // BLOCK if nrows > 0 else -1
        wf = wave_of(nb_w, first) if nrows > 0 else 0
        wl = wave_of(nb_w, last) if nrows > 0 else -1
        part_off = words
        words += (wl - wf + 1) * slots * S
        aux_off = words
        words += naux * S
        seg_plans.append(dict(first_block=first, last_block=last, wave_first=wf, wave_last=wl, part_off=part_off,
                              aux_off=aux_off))
    return words, seg_plans


def plan(n, k, n_rows, out_identity, segs, samples=0):
    """The header's ``wide_fused64_plan`` in Python: (plan dict, list of per-segment dicts).  ``samples``: 0 (32 where the
    LDS fits, else 16), or 16 / 32 forced."""
    kp = (n + 7) // 8 * 8
    ks = kp + 2
    rows_w_pad = (n_rows + 15) // 16 * 16
    nb_w = rows_w_pad // 16
    rows_e_pad = 0 if out_identity else (k + 15) // 16 * 16
    envelope = 1 <= n <= MAX_N and k >= 1 and samples in (0, 16, 32)
    for S in ((16,) if samples == 16 else (32,) if samples == 32 else (32, 16)):
        words, seg_plans = _scratch(nb_w, S, segs)
        tile_bytes = 8 * S * ks
        lds = tile_bytes + 8 * words + 8 * 2 * S
        served = int(envelope and lds <= LDS)
        if served:
            break
    p = dict(n=n, kp=kp, ks=ks, samples=S, rows_w_pad=rows_w_pad, nb_w=nb_w, rows_e_pad=rows_e_pad, nb_e=rows_e_pad // 16,
             rows_pad=rows_w_pad + rows_e_pad, scratch_words=words, tile_bytes=tile_bytes, lds_bytes=lds, served=served)
    return p, seg_plans


PLAN_KEYS = ("n", "kp", "ks", "samples", "rows_w_pad", "nb_w", "rows_e_pad", "nb_e", "rows_pad", "scratch_words", "tile_bytes",
             "lds_bytes", "served")


def plan_of(c, samples=0):
    """The restated plan of a pack (``PackedConstants``)."""
    return plan(c.n, c.k, c.W.shape[0], int(c.out_identity), seg_inputs(c.segments), samples)


# ---------------------------------------------------------------- the sets
def _edge_raw(n):
    """The family of ``s32_last`` / ``s16_first``: 20 linear rows and a cone of 5, whatever n (so the scratch is too)."""
    return workloads.random_lin_quad_soc(k=n, m=20, n_quad=0, n_soc=1, r_M=5, seed=96)


@functools.lru_cache(maxsize=None)
def s32_last_n():
    """The largest n of the ``_edge_raw`` family whose plan picks 32 samples: searched with the restated plan on the
    family's segment table (which does not depend on n: checked by tests/test_wide_fused64_host.py on the sets built)."""
    from rayen_amd.constraint_module import ConstraintModule
    c = ConstraintModule(workloads.build_constraints(_edge_raw(70)), create_map=False).packed_constants()
    segs, rows = seg_inputs(c.segments), c.W.shape[0]
    picks = [n for n in range(65, MAX_N + 1) if plan(n, n, rows, 1, segs)[0]["samples"] == 32]
    assert picks and picks == list(range(65, picks[-1] + 1)) and picks[-1] < MAX_N
    return picks[-1]


@functools.lru_cache(maxsize=None)
def raw(name):
    if name == "n65":
        return workloads.random_lin_quad_soc(k=65, m=17, n_quad=1, n_soc=1, r_M=17, seed=191)
    if name == "n66_one_row":
        return workloads.random_lin_quad_soc(k=66, m=1, n_quad=0, n_soc=0, seed=192)
    if name in ("k190_n160", "k1024", "k1025"):
        return F.raw(name)
    if name == "s32_last":
        return _edge_raw(s32_last_n())
    if name == "s16_first":
        return _edge_raw(s32_last_n() + 1)
    if name == "n64":                   # the last n below the wide route in fp64 (the no-effect test)
        return workloads.random_lin_quad_soc(k=64, m=30, n_quad=1, n_soc=1, r_M=10, seed=193)
    if name == "plan_a":
        r = workloads.random_lin_quad_soc(k=70, m=20, n_quad=0, n_soc=2, r_M=20, seed=194)
        WS._low_rank(r, 70, np.random.default_rng(1194), 10, 0.1)
        return WS._tighten(r, (4.0,), (2.2, 2.2))
    if name in PLAN_B:
        return workloads.random_lin_quad_soc(k=70, m=PLAN_B[name], n_quad=0, n_soc=1, r_M=5, seed=400 + PLAN_B[name])
    if name == "plan_c":
        r = workloads.random_lin_quad_soc(k=70, m=20, n_quad=0, n_soc=0, seed=195)
        rng = np.random.default_rng(1195)
        for rows in FAC_ROWS:
            WS._low_rank(r, 70, rng, rows - 1, 0.1)
        return WS._tighten(r, (3.0, 2.0, 3.0, 3.0), ())
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def cs(name):
    return WS.cs(_FROM_SWEEP[name]) if name in _FROM_SWEEP else workloads.build_constraints(raw(name))


@functools.lru_cache(maxsize=None)
def packed(name):
    """The packer's own layout of a case's set."""
    from rayen_amd.constraint_module import ConstraintModule
    return ConstraintModule(cs(name), create_map=False).packed_constants()


@functools.lru_cache(maxsize=None)
def consts(name):
    """The pack of a case: the packer's layout (``OWN``) or the relaid one."""
    if name in _FROM_SWEEP:
        return WS.consts(_FROM_SWEEP[name])
    p = packed(name)
    if name == "plan_a":
        (fac,), (soc_a, soc_b) = WS._by_type(p, _lib.SEG_QUAD_FAC), WS._by_type(p, _lib.SEG_SOC)
        return WS.relayout(p, order=[fac, soc_a, soc_b, 0], gaps={("after", fac): 15 - (1 + p.segments[fac].nrows)})
    if name in PLAN_B:
        return WS.relayout(p, order=[1, 0])
    if name == "plan_c":
        fac = WS._by_type(p, _lib.SEG_QUAD_FAC)
        assert [p.segments[i].nrows for i in fac] == list(FAC_ROWS)
        return WS.relayout(p, gaps={("after", 0): 5})
    return p


def inputs(name, batch=B):
    """``[batch, n]`` fp64 (the sweep's own inputs for the sets taken from it)."""
    if name in _FROM_SWEEP:
        return WS.inputs(_FROM_SWEEP[name])[:batch, :, 0].double()
    n = consts(name).n
    x = F.inputs(n, batch)[:, :, 0].double()
    x[9:] *= SCALE
    return x


@functools.lru_cache(maxsize=None)
def truth(name):
    """(y64, kappa64, active64) of a case on its pack, in fp64 on the host; computed once and left unchanged."""
    out = WS.evaluate64(consts(name), inputs(name).numpy())
    for a in out:
        a.setflags(write=False)
    return out
