"""The re-laying of a projection program's rows for the tile kernel (rayen_amd/csrc/rayen_proj_tile.hip: ``tile_layout``),
restated independently of the C++ in Python integers.  ``tests/test_proj_tile_host.py`` holds
``rayen_proj_tile_layout`` against it.

Blocks of 32 rows, four waves, wave ``w`` a contiguous range of whole blocks.  ``nb`` is the smallest number of blocks per
wave at which this holds: the cones, in their order, go to waves 0, 1, .. (a cone that no longer fits the ``32 nb`` rows of
a wave opens the next); each wave's cones lie back to back at the start of its range, padded to whole blocks; the orthant
rows then fill what the cones left, wave 0 first, each wave's share padded to a whole block.  Pads are -1."""
WAVES, BLOCK = 4, 32
MAX_BLOCKS = 12                       # blocks per wave the largest instance holds (n <= 32; 10 above)
MAX_ROWS = WAVES * BLOCK * MAX_BLOCKS


def max_blocks(n):
    return 12 if n <= 32 else 10


def layout(m_lin, soc_rows, limit=MAX_BLOCKS):
    """``(Mp, perm [Mp], first_block [5], nb)`` or ``None`` when no ``nb <= limit`` holds the rows."""
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
            return len(perm), perm, first, nb
    return None
