"""The scratch-buffer sizes of the DC3 and projection layers, restated independently of the C++ in Python integers.
``tests/test_side_layout_host.py`` holds ``rayen_side_layout.h`` against them and ``tests/test_gpu_side_ops_contract.py`` the
library's ``rayen_*_workspace_bytes``.

Every region is a whole number of 256-byte lines.  ``(total, [offset of each region])``."""
BATCHES = (0, 1, 255, 4097)
STEPS = (1, 32, 33)
DC3_CHUNK = 32               # steps per launch (rayen_dc3.hip: kChunk)
DC3_VIOL_BYTES = 8           # one slot per step, wide enough for the bits of a double


def align256(x):
    return (x + 255) // 256 * 256


def dc3_forward(n, B, max_steps, elem):
    """viol [max_steps + 1] | with more than one chunk of steps: two states [2 n][B] (none otherwise)."""
    viol = align256((max_steps + 1) * DC3_VIOL_BYTES)
    state = align256(2 * n * B * elem) if -(-max_steps // DC3_CHUNK) > 1 else 0
    return viol + 2 * state, [0, viol, viol + state]


def dc3_backward(n, B, max_steps, elem):
    """the recomputed trajectory [max_steps][n][B]"""
    return align256(max_steps * n * B * elem), [0]


def proj(n, m, B, elem, backward):
    """x [B][n] | status [B] int32 | backward: its v [B][m]"""
    xs, status = align256(B * n * elem), align256(B * 4)
    total = xs + status + (align256(B * m * elem) if backward else 0)
    return total, [0, xs, xs + status]
