"""The streamed Bar kernels' cases (rayen_amd/csrc/rayen_bar_stream.hip): the forced window sizes of every sweep case and
a Python restatement of rayen_amd/csrc/rayen_bar_stream_layout.h, which tests/test_bar_stream_host.py holds against the
header itself (a host-only C++ probe) and tests/test_gpu_bar_stream.py reads its batch sizes from.

Nothing here imports ``rayen_amd``.
"""
import bar_reference as br

DTYPES = ("float32", "float64")
ELEM = {"float32": 4, "float64": 8}

# ---- rayen_bar_stream_layout.h, restated
LDS = 160 * 1024
YP_BYTES = 64 * 8
THREADS = 512
MAX_WINDOW = (LDS - YP_BYTES) // 2 // 16 * 16
DEFAULT_WINDOW = 20 * 1024


def window_ok(window_bytes):
    return window_bytes == 0 or (window_bytes > 0 and window_bytes % 16 == 0 and window_bytes <= DEFAULT_WINDOW)


def groups(window_bytes, K, elem):
    return (window_bytes or DEFAULT_WINDOW) // (4 * K * elem)


def pieces(m):
    return (m + 3) // 4


def windows(m, g):
    return (pieces(m) + g - 1) // g


def window_of(piece, g):
    return piece // g


def buffer_bytes(m, g, K, elem):
    return min(pieces(m), g) * 4 * K * elem


def lds_bytes(m, g, K, elem):
    return YP_BYTES + (2 if windows(m, g) > 1 else 1) * buffer_bytes(m, g, K, elem)


def vertex_windows(nv, g):
    return (pieces(nv) - 1) // g + 1 if nv > 0 else 0


def forward_seq(nv, m, g):
    nw = windows(m, g)
    return list(range(vertex_windows(nv, g))) + list(range((nv // 4) // g if m > nv else nw, nw))


def backward_seq(nv, m, g):
    return list(range(vertex_windows(nv, g))) + list(range(windows(m, g)))


def group_log2(m):
    lg = 0
    while (1 << lg) < pieces(m) and lg < 4:
        lg += 1
    return lg


def rows(K, f64):
    """R: rows a lane group carries at once (rayen_bar_stream_layout.h: bar_stream_rows)."""
    return 1


def rows_per_pass(m, K, f64):
    return (THREADS >> group_log2(m)) * rows(K, f64)


def wg_per_cu(lds):
    return max(1, min(4, LDS // lds))


def copies(seq, passes=1):
    """Windows a workgroup copies over ``passes`` passes of ``seq``: a step whose window is the previous step's copies
    nothing."""
    steps = seq * passes
    return sum(1 for i, w in enumerate(steps) if i == 0 or steps[i - 1] != w)


# ---- the forced windows of a case

def forced_windows(case, dtype_name):
    """(a) one group of four generators: every piece its own window; (b) three groups: a boundary falls inside an L-round
    and, where the case has one, next to the mixed vertex / ray piece; (c) the smallest legal size that holds the whole image
    (one window, the buffer stays) -- where the image is larger than the largest legal window, that window; (d) 0, the
    default."""
    K, elem = br.pad_k(case.k), ELEM[dtype_name]
    group = 4 * K * elem
    return [group, 3 * group, min(pieces(case.nv + case.nr) * group, DEFAULT_WINDOW // group * group), 0]


def whole_image_fits(case, dtype_name):
    return pieces(case.nv + case.nr) * 4 * br.pad_k(case.k) * ELEM[dtype_name] <= DEFAULT_WINDOW


def window_count(case, dtype_name, window_bytes):
    return windows(case.nv + case.nr, groups(window_bytes, br.pad_k(case.k), ELEM[dtype_name]))


JOBS = [(case, dtype_name, w) for case in br.CASES for dtype_name in DTYPES for w in forced_windows(case, dtype_name)]
assert all(window_ok(w) and groups(w, br.pad_k(c.k), ELEM[d]) >= 1 for c, d, w in JOBS)
_counts = {window_count(c, d, w) for c, d, w in JOBS}
assert any(n > 1 and n % 2 for n in _counts) and any(n > 1 and n % 2 == 0 for n in _counts), _counts
assert all((window_count(c, d, forced_windows(c, d)[2]) == 1) == whole_image_fits(c, d) for c in br.CASES for d in DTYPES)
# one window (the buffer stays) at every K and L, and several windows of the default size somewhere in each precision
assert {(br.pad_k(c.k), br.lanes(c.nv + c.nr)) for c in br.CASES if whole_image_fits(c, "float64")} >= \
    {(4, 1), (8, 2), (16, 4), (32, 8), (64, 16), (4, 16), (16, 16)}
assert all(any(window_count(c, d, 0) > 1 for c in br.CASES) for d in DTYPES)
# (b) really cuts inside an L-round somewhere, and next to a mixed piece somewhere
assert any(br.lanes(c.nv + c.nr) > 3 and window_count(c, "float32", forced_windows(c, "float32")[1]) > 1 for c in br.CASES)
assert any(c.nv % 4 and c.nr and (c.nv // 4) % 3 in (0, 2) and pieces(c.nv + c.nr) > 3 for c in br.CASES)
