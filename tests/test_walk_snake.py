"""The serpentine top level of the lattice brick walk (csrc/fuse_common.h: walk_tile with EvalParams::walk_snake, set by the
channel-sliced family only): a Python mirror of the closed form, checked to be a permutation of the tiles of a lattice --
every tile exactly once, clipped blocks included -- and to be what it is for: consecutive macro-bricks of the walk share a
face, where the row-major order jumps back at the end of every row.  The levels below the macro-bricks are untouched.
walk_tile itself is device code with no host-callable form; on the device the coverage is the sentinel check of
tests/test_gpu_sliced_dead_pairs.py (every output element written, results equal to the caller-order launch)."""
import pytest


def snake_index(rem, full, first, rev):
    """position j of the block holding `rem` when the blocks hold `full` items each except the clipped one (`first` items),
    which a reversed walk meets FIRST; returns (j, rem inside the block)"""
    if not rev or rem < first:
        j = 0 if rev else rem // full
        return j, rem - (0 if rev else j * full)
    r = rem - first
    j = 1 + r // full
    return j, r - (j - 1) * full


def walk_level(rem, b, box, snake=False):
    """mirror of walk_level / walk_level_snake: box = (ox, oy, oz, ex, ey, ez) in tiles; returns (rem, box of the block)"""
    ox, oy, oz, ex, ey, ez = box
    slab = b * ey * ez
    i = rem // slab
    rem -= i * slab
    bx = min(b, ex - i * b)
    ney, nez = (ey + b - 1) // b, (ez + b - 1) // b
    j, rem = snake_index(rem, bx * b * ez, bx * (ey - (ney - 1) * b) * ez, snake and i % 2 == 1)
    jc = ney - 1 - j if (snake and i % 2 == 1) else j
    by = min(b, ey - jc * b)
    rev_z = snake and (i * ney + j) % 2 == 1
    k, rem = snake_index(rem, bx * by * b, bx * by * (ez - (nez - 1) * b), rev_z)
    kc = nez - 1 - k if rev_z else k
    return rem, (ox + i * b, oy + jc * b, oz + kc * b, bx, by, min(b, ez - kc * b))


def walk_tile(dims, tile, t, snake):
    """tile coordinates (x, y, z) of walk position t, and the macro-brick it lies in"""
    e = [(dims[a] + tile[a] - 1) // tile[a] for a in range(3)]
    rem, box = walk_level(t, 16, (0, 0, 0, e[0], e[1], e[2]), snake)
    macro = (box[0] // 16, box[1] // 16, box[2] // 16)
    rem, box = walk_level(rem, 8, box)
    rem, box = walk_level(rem, 4, box)
    ox, oy, oz, ex, ey, ez = box
    lx, r2 = divmod(rem, ey * ez)
    ly, lz = divmod(r2, ez)
    return (ox + lx, oy + ly, oz + lz), macro


DIMS = [((70, 70, 17), (2, 2, 1)), ((33, 35, 61), (2, 2, 1)), ((5, 7, 3), (2, 2, 1)), ((32, 32, 16), (2, 2, 1)), ((97, 33, 70), (2, 2, 2)),
        ((130, 66, 40), (2, 2, 1)), ((66, 131, 45), (2, 2, 2)), ((34, 98, 33), (2, 2, 1)), ((1, 1, 1), (2, 2, 1)), ((40, 36, 200), (2, 2, 4))]


@pytest.mark.parametrize("dims,tile", DIMS)
def test_serpentine_walk_is_a_permutation_of_the_tiles(dims, tile):
    e = [(dims[a] + tile[a] - 1) // tile[a] for a in range(3)]
    n = e[0] * e[1] * e[2]
    plain = [walk_tile(dims, tile, t, False) for t in range(n)]
    snake = [walk_tile(dims, tile, t, True) for t in range(n)]
    for walk in (plain, snake):
        tiles = [w[0] for w in walk]
        assert len(set(tiles)) == n and all(0 <= c[a] < e[a] for c in tiles for a in range(3))
    # the same macro-bricks with the same contents in the same inner order: only the order of the macro-bricks differs
    def by_macro(walk):
        d = {}
        for c, m in walk:
            d.setdefault(m, []).append(c)
        return d
    assert by_macro(plain) == by_macro(snake)
    # consecutive macro-bricks of the serpentine share a face
    seq = [m for q, (c, m) in enumerate(snake) if q == 0 or snake[q - 1][1] != m]
    assert len(seq) == len(set(seq))
    assert all(sum(abs(a - b) for a, b in zip(seq[q], seq[q + 1])) == 1 for q in range(len(seq) - 1)), seq
