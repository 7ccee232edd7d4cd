"""The re-laying of a projection program's rows for the fp64 tile kernel (rayen_amd/csrc/rayen_proj_tile64_layout.h), its
instances and its LDS bytes, restated independently of the C++ in Python integers.  ``tests/test_proj_tile64_host.py``
holds ``rayen_proj_tile64_layout`` against it.

``tests/tile_layout_formulas.py``'s rule with blocks of 16 rows: four waves, wave ``w`` a contiguous range of whole blocks.
``nb`` is the smallest number of blocks per wave at which this holds: the cones, in their order, go to waves 0, 1, .. (a
cone that no longer fits the ``16 nb`` rows of a wave opens the next); each wave's cones lie back to back at the start of its
range, padded to whole blocks; the orthant rows then fill what the cones left, wave 0 first, each wave's share padded to a
whole block.  Pads are -1."""
WAVES, BLOCK = 4, 16
MAX_BLOCKS = 24                       # blocks per wave the largest instance holds (n <= 32; 20 above)
MAX_ROWS = WAVES * BLOCK * MAX_BLOCKS
MAX_N, MAX_CONES = 64, 4096
BLOCK_BYTES = BLOCK * BLOCK * 8       # one block's LDS image; one block of registers parked in LDS
FIXED_BYTES = 1024 + 256
LDS_LIMIT = 160 * 1024 - 256


def max_blocks(n):
    return 24 if n <= 32 else 20


def instance(nb, n):
    """(NB, NX) of the kernel instance that runs a layout of ``nb`` blocks a wave at ``n`` variables."""
    nx = 2 if n <= 32 else 4
    return (4 if nb <= 4 else 12 if nb <= 12 else 24 if nx == 2 else 20), nx


def parked(NB):
    """Blocks of p an instance keeps in LDS."""
    return 6 if NB > 20 else 2 if NB == 20 else 0


def layout(m_lin, soc_rows, limit=MAX_BLOCKS):
    """``(Mp, perm [Mp], first_block [5], nb, cone_blocks [4])`` or ``None`` when no ``nb <= limit`` holds the rows."""
    for nb in range(1, limit + 1):
        cap = BLOCK * nb
        waves = [[] for _ in range(WAVES)]
        used = [0] * WAVES
        w = 0
        for c, rows in enumerate(soc_rows):
            while w < WAVES and used[w] + rows > cap:
                w += 1
            if w == WAVES:
                break
            waves[w].append(c)
            used[w] += rows
        else:
            cone_blocks = [-(-u // BLOCK) for u in used]
            if sum(cap - BLOCK * cb for cb in cone_blocks) < m_lin:
                continue
            start = [m_lin]
            for rows in soc_rows:
                start.append(start[-1] + rows)
            perm, first, orth = [], [], 0
            for k in range(WAVES):
                first.append(len(perm) // BLOCK)
                for c in waves[k]:
                    perm += list(range(start[c], start[c + 1]))
                perm += [-1] * (BLOCK * cone_blocks[k] - used[k])
                take = min(m_lin - orth, cap - BLOCK * cone_blocks[k])
                perm += list(range(orth, orth + take))
                orth += take
                perm += [-1] * (-take % BLOCK)
            first.append(len(perm) // BLOCK)
            return len(perm), perm, first, nb, cone_blocks
    return None


def lds_bytes(n, m_lin, soc_rows, backward=True):
    """Dynamic LDS of a launch, or ``None`` without a layout: the cone blocks' images (which the four waves' partial sums
    of G'u reuse), v*'s cone images (backward), 2q + w0, the fixed part, perm, the parked blocks of p."""
    lay = layout(m_lin, soc_rows, max_blocks(n))
    if lay is None:
        return None
    Mp, _, _, nb, cone_blocks = lay
    NB, nx = instance(nb, n)
    cones = sum(cone_blocks) * BLOCK_BYTES
    shared = max(cones, WAVES * nx * BLOCK_BYTES)
    return shared + (cones if backward else 0) + nx * BLOCK_BYTES + FIXED_BYTES + 4 * Mp + WAVES * parked(NB) * BLOCK_BYTES


def served(n, m_lin, soc_rows):
    """``tile64_served()`` for a program without a PSD block."""
    if not 1 <= n <= MAX_N or len(soc_rows) > MAX_CONES or m_lin < 0 or any(r < 1 for r in soc_rows):
        return False
    m = m_lin + sum(soc_rows)
    if m < 1 or m > MAX_ROWS:
        return False
    need = lds_bytes(n, m_lin, soc_rows)
    return need is not None and need <= LDS_LIMIT
