"""Host-side emulation of the two NaN / Inf row flags of the W-in-LDS schedule (rayen_amd/csrc/rayen_mfma_pair_wl.hip): the
instances without screening fold the row's leading f16 pieces (pair_nan_fold: z <- p1 * 0 + z, NaN once a piece is infinite or
NaN), the screening instances test nv2 = ||sv v||^2, the fp32 sum of the 64 scaled squares they need anyway:
nan_row = !(nv2 < inf).  Both must say "a component of the row is NaN or infinite", nothing else: the scaling is the kernel's
(pow2_scale: exponent arithmetic on the row's largest |component|, fmaxf ignoring NaNs, the biased exponent clamped to
[14, 254]), the pieces and the sum are formed in the kernel's order (two FMA chains per half row, the chains added, the halves
added).  No GPU."""
import numpy as np
import pytest

N = 64


def _pow2_scale(m):
    """rayen_split_image.h::pow2_scale: 2^13 / 2^floor(log2 m) from the biased exponent of m, clamped to [14, 254]."""
    e = np.float32(m).view(np.uint32) >> np.uint32(23)
    e = np.clip(e, 14, 254).astype(np.uint32)
    return (np.uint32(267) - e << np.uint32(23)).view(np.float32)


def _row_max(v):
    """half_max + the exchange: a running fmaxf over |components| from 0 (fmaxf returns the other operand for a NaN)."""
    with np.errstate(invalid="ignore"):
        return np.float32(np.fmax.reduce(np.abs(v), initial=np.float32(0)))


def _fma32(a, b, c):
    """fl32(a * b + c), one rounding (the product of two fp32 values is exact in fp64; so is its sum with an fp32 value below
    2^40 in magnitude here, up to the final rounding -- non-finite operands propagate as in hardware)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def _flag_by_fold(v):
    """pair_nan_fold over the leading pieces p1 = f16(v sv) of the whole row (both halves end in one OR)."""
    sv = _pow2_scale(_row_max(v))
    with np.errstate(invalid="ignore", over="ignore"):
        p1 = (v.astype(np.float32) * sv).astype(np.float16)
        z = np.float16(0)
        for p in p1:
            z = np.float16(p * np.float16(0) + z)
    return bool(np.isnan(z)), p1


def _flag_by_nv2(v):
    sv = _pow2_scale(_row_max(v))
    halves = []
    for hi in (0, 1):
        s0 = s1 = np.float32(0)
        for q in range(N // 8):                      # the lane's pieces 2 q + hi: columns 8 q + 4 hi .. + 3
            for c in (0, 2):
                with np.errstate(invalid="ignore", over="ignore"):
                    x0 = np.float32(v[8 * q + 4 * hi + c] * sv)
                    x1 = np.float32(v[8 * q + 4 * hi + c + 1] * sv)
                s0 = _fma32(x0, x0, s0)
                s1 = _fma32(x1, x1, s1)
        with np.errstate(invalid="ignore", over="ignore"):
            halves.append(np.float32(s0 + s1))
    with np.errstate(invalid="ignore", over="ignore"):
        nv2 = np.float32(halves[0] + halves[1])
    return (not bool(nv2 < np.float32(np.inf))), nv2


def _edge_rows():
    rng = np.random.default_rng(5)
    base = rng.uniform(-1.5, 1.5, size=N).astype(np.float32)
    tiny, big = np.float32(1e-20), np.float32(1e20)
    f32 = np.finfo(np.float32)
    rows = {"ordinary": base, "1e20": base * big, "1e-20": base * tiny, "zero": np.zeros(N, np.float32),
            "largest finite everywhere": np.full(N, f32.max, np.float32), "largest finite once": base.copy(),
            "smallest normal everywhere": np.full(N, f32.tiny, np.float32),
            "subnormal everywhere": np.full(N, np.float32(1e-45), np.float32),
            "one component, rest zero": np.zeros(N, np.float32), "negative zero": np.full(N, -0.0, np.float32),
            "powers of two just below 2^14 after scaling": np.full(N, np.float32(1.9999999), np.float32)}
    rows["largest finite once"][17] = f32.max
    rows["one component, rest zero"][63] = np.float32(-3.5)
    bad = {}
    for name, val in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        for col in (0, 5, 36, 63):                   # both halves of the row, first and last piece
            for host in ("ordinary", "1e20", "1e-20", "zero"):
                r = rows[host].copy()
                r[col] = val
                bad[f"{name} at {col} in a {host} row"] = r
    allnan = np.full(N, np.nan, np.float32)
    mixed = base.copy()
    mixed[3], mixed[40] = np.inf, -np.inf
    bad["every component NaN"] = allnan
    bad["+inf and -inf"] = mixed
    bad["every component +inf"] = np.full(N, np.inf, np.float32)
    return rows, bad


_FINITE, _BAD = _edge_rows()


@pytest.mark.parametrize("name", sorted(_FINITE))
def test_a_finite_row_raises_neither_flag(name):
    v = _FINITE[name]
    fold, p1 = _flag_by_fold(v)
    by_nv2, nv2 = _flag_by_nv2(v)
    # (the scaled fp32 values are below 2^14; rounding to f16 can reach 2^14 itself, far from the format's 65 504)
    assert np.isfinite(p1.astype(np.float64)).all() and np.abs(p1.astype(np.float64)).max() <= 2.0 ** 14
    assert np.isfinite(nv2) and nv2 < 2.0 ** 34      # (64 squares below 2^28: the sum cannot overflow)
    assert fold is False and by_nv2 is False


@pytest.mark.parametrize("name", sorted(_BAD))
def test_a_row_with_a_nan_or_an_infinite_component_raises_both_flags(name):
    v = _BAD[name]
    fold, _ = _flag_by_fold(v)
    by_nv2, nv2 = _flag_by_nv2(v)
    assert fold is True and by_nv2 is True, (fold, by_nv2, nv2)


def test_random_rows_of_every_magnitude_agree():
    rng = np.random.default_rng(11)
    for i in range(300):
        v = (rng.uniform(-1.5, 1.5, size=N) * 10.0 ** rng.integers(-38, 38)).astype(np.float32)
        if i % 3 == 0:
            v[rng.integers(0, N)] = (np.nan, np.inf, -np.inf)[(i // 3) % 3]
        want = not bool(np.isfinite(v).all())
        assert _flag_by_fold(v)[0] == want and _flag_by_nv2(v)[0] == want
