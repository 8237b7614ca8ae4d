"""The lattice walk's decode (csrc/fuse_common.h: walk_tile) for every value of EvalParams::walk_snake -- 0: three blocked levels
(16-tile macro-bricks, 8-tile sub-bricks, 4-tile mini-bricks), each row-major; 1: the macro-bricks as a serpentine (the
channel-sliced family on fp32 maps).  A NumPy restatement of the closed form (the same integer arithmetic, vectorised over the
walk positions; walk_level takes the serpentine flag per level, so the restatement also covers the lower levels, which were
built, measured and not kept: DESIGN.md 5.5), checked to be a bijection of the tile lattice, to leave the levels it does not
flip exactly as they were, and to be what it is for: consecutive blocks of a flipped level that lie in the same parent share
a face -- the clipped blocks at the upper faces included, which a reversed row meets first.  Lattices: a single tile, a
column, one clipped mini-brick, one clipped at every level, and one with more than one macro-brick on every axis and odd
counts.  walk_tile itself is device code; on the device the coverage is tests/test_gpu_sliced_walk_order.py."""
import numpy as np
import pytest

LEVELS = (16, 8, 4)


def snake_index(rem, full, last, rev):
    """walk_snake_index: position of the block holding `rem` along one axis and the position inside that block; the blocks
    hold `full` positions each, except the clipped one (`last` positions), which a reversed walk meets first"""
    j_fwd = rem // full
    r_fwd = rem - j_fwd * full
    first = rem < last
    r2 = rem - last
    j_rev = np.where(first, 0, r2 // full + 1)
    r_rev = np.where(first, rem, r2 - (r2 // full) * full)
    return np.where(rev, j_rev, j_fwd), np.where(rev, r_rev, r_fwd)


def walk_level(rem, b, o, e, snake):
    """walk_level (snake False) / walk_level_snake (True) for arrays of positions: o, e = [3] arrays of origins / extents"""
    ox, oy, oz = o
    ex, ey, ez = e
    slab = b * ey * ez
    i = rem // slab
    rem = rem - i * slab
    bx = np.minimum(b, ex - i * b)
    ny, nz = (ey + b - 1) // b, (ez + b - 1) // b
    rev_y = (i % 2 == 1) & snake
    j, rem = snake_index(rem, bx * b * ez, bx * (ey - (ny - 1) * b) * ez, rev_y)
    jc = np.where(rev_y, ny - 1 - j, j)
    by = np.minimum(b, ey - jc * b)
    rev_z = ((i * ny + j) % 2 == 1) & snake
    k, rem = snake_index(rem, bx * by * b, bx * by * (ez - (nz - 1) * b), rev_z)
    kc = np.where(rev_z, nz - 1 - k, k)
    return rem, (ox + i * b, oy + jc * b, oz + kc * b), (bx, by, np.minimum(b, ez - kc * b))


def walk_tiles(e_tiles, walk_snake):
    """tile coordinates [n, 3] of every walk position, and per level the origin [n, 3] of the block the position lies in"""
    n = e_tiles[0] * e_tiles[1] * e_tiles[2]
    rem = np.arange(n, dtype=np.int64)
    zero = np.zeros(n, np.int64)
    o = (zero, zero, zero)
    e = tuple(zero + x for x in e_tiles)
    blocks = []
    for lvl, b in enumerate(LEVELS):
        rem, o, e = walk_level(rem, b, o, e, walk_snake > lvl)
        blocks.append(np.stack(o, 1))
    yz = e[1] * e[2]
    lx = rem // yz
    r2 = rem - lx * yz
    ly = r2 // e[2]
    lz = r2 - ly * e[2]
    return np.stack((o[0] + lx, o[1] + ly, o[2] + lz), 1), blocks


VALUES = (0, 1)                     # the values the kernels know; 2 and 3 (sub- and mini-bricks too) are what was tried
LATTICES = [(1, 1, 1), (1, 5, 1), (3, 3, 3), (17, 9, 33), (33, 17, 35)]


@pytest.fixture(scope="module")
def walks():
    return {(e, s): walk_tiles(e, s) for e in LATTICES for s in VALUES}


@pytest.mark.parametrize("walk_snake", VALUES)
@pytest.mark.parametrize("e_tiles", LATTICES)
def test_walk_is_a_bijection_of_the_tile_lattice(walks, e_tiles, walk_snake):
    tiles, _ = walks[(e_tiles, walk_snake)]
    n = e_tiles[0] * e_tiles[1] * e_tiles[2]
    assert tiles.shape == (n, 3)
    assert (tiles >= 0).all() and (tiles < np.asarray(e_tiles)).all()
    flat = (tiles[:, 0] * e_tiles[1] + tiles[:, 1]) * e_tiles[2] + tiles[:, 2]
    assert len(np.unique(flat)) == n


def runs(keys):
    """first position of every run of equal rows"""
    change = np.ones(len(keys), bool)
    change[1:] = (keys[1:] != keys[:-1]).any(axis=1)
    return np.flatnonzero(change)


@pytest.mark.parametrize("walk_snake", VALUES)
@pytest.mark.parametrize("e_tiles", LATTICES)
def test_blocks_hold_what_they_held_and_flipped_levels_step_to_face_neighbours(walks, e_tiles, walk_snake):
    tiles, blocks = walks[(e_tiles, walk_snake)]
    plain_tiles, plain_blocks = walks[(e_tiles, 0)]
    for lvl, b in enumerate(LEVELS):
        # a block of the walk is a contiguous stretch of positions, visited once, and lies where its origin says
        key = np.concatenate(blocks[:lvl + 1], axis=1)
        starts = runs(key)
        assert len(np.unique(key[starts], axis=0)) == len(starts)
        assert ((tiles >= blocks[lvl]) & (tiles < blocks[lvl] + b)).all()
        assert (blocks[lvl] % b == 0).all()
        # consecutive blocks of a flipped level inside one parent share a face: one block step along one axis
        if walk_snake > lvl:
            parent = key[starts][:, :3 * lvl]
            same_parent = (parent[1:] == parent[:-1]).all(axis=1) if lvl else np.ones(len(starts) - 1, bool)
            step = np.abs(np.diff(blocks[lvl][starts], axis=0)).sum(axis=1)
            assert (step[same_parent] == b).all(), (lvl, step[same_parent])
    # the same tiles in every mini-brick, in the same (row-major) order inside it: only the order of the blocks differs
    def by_mini(t, bl):
        order = np.lexsort((np.arange(len(t)), bl[2][:, 2], bl[2][:, 1], bl[2][:, 0]))
        return np.concatenate((bl[2], t), axis=1)[order]
    assert np.array_equal(by_mini(tiles, blocks), by_mini(plain_tiles, plain_blocks))


def test_value_0_is_the_blocked_row_major_order_and_the_lower_levels_would_be_bijections_too():
    """walk_snake 0 against a plain sort key; and the restatement with the sub- and mini-bricks flipped as well (2, 3: measured,
    not kept) is still a bijection that walks the macro-bricks in the order of 1"""
    e = (33, 17, 35)
    tiles, _ = walk_tiles(e, 0)
    g = np.stack(np.meshgrid(*[np.arange(x) for x in e], indexing="ij"), -1).reshape(-1, 3)
    keys = [g[:, a] // b for b in (16, 8, 4, 1) for a in range(3)]          # most significant first
    assert np.array_equal(tiles, g[np.lexsort(keys[::-1])])
    _, blocks1 = walk_tiles(e, 1)
    for value in (2, 3):
        t, blocks = walk_tiles(e, value)
        assert len(np.unique((t[:, 0] * e[1] + t[:, 1]) * e[2] + t[:, 2])) == len(g)
        assert np.array_equal(blocks1[0], blocks[0])
