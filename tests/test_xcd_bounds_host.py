"""The cut rule of the walk's balance mode, restated on the host (tests/xcd_ref.py), has the covering property from 8
blocks on and loses it below: the recorded reason for the gate in enqueue_walk and for what the two debug hooks refuse.

The property (xcd_ref.covers_once): the workgroups (xcd, jb < jmax) with bounds[xcd] + jb < bounds[xcd + 1] walk every
logical block 0 .. nb - 1 exactly once.  A block no range covers keeps the other buffer's stale state; a block two
ranges cover is integrated twice.  The checker lists the blocks walked and knows nothing of the clamps.

tests/test_gpu_xcd_balance.py holds the device's k_xcd_bounds to these functions, bound by bound.
"""
import numpy as np
import pytest

import xcd_ref as X

BIG = (8191, 8192, 39_063, 117_188)       # around the default threshold (2 M bodies), 10 M and 30 M bodies
LOOP_NB = tuple(range(8, 200)) + (1023, 1024, 1025, 2047, 2049, 4096, 39_063)  # chunk 1, 2, 3, 4 and 39
CHUNKS = (-1, 0, 1, 2, 3, 5, 64)


def _check(nb):
    jm = X.jmax(nb)
    assert 8 * jm >= nb
    for name, table in X.patterns(nb):
        b = X.bounds(table)
        assert b[0] == 0 and b[8] == nb, (nb, name, b)
        widths = np.diff(b)
        assert widths.min() >= 1 and widths.max() <= jm, (nb, name, b, jm)
        assert X.covers_once(b, nb, jm), (nb, name, b, jm)


@pytest.mark.parametrize("lo,hi", [(8, 1400), (1400, 2800), (2800, 4201)])
def test_bounds_cover_every_block_once(lo, hi):
    for nb in range(lo, hi):
        _check(nb)


@pytest.mark.parametrize("nb", BIG)
def test_bounds_cover_every_block_once_large(nb):
    _check(nb)


def test_searchsorted_cut_equals_the_kernels_loop():
    for nb in LOOP_NB:
        for name, table in X.patterns(nb):
            assert X.raw_cuts(table) == X.raw_cuts_loop(table), (nb, name)


def test_the_patterns_reach_every_clamp():
    """The clamps are what only skewed times reach: each of the four changes a cut in some pattern at some size."""
    fired = set()
    for nb in (8, 9, 17, 100, 1025, 8192):
        jm = X.jmax(nb)
        for _, table in X.patterns(nb):
            prev = 0
            for k, c in enumerate(X.raw_cuts(table), start=1):
                if c < prev + 1:
                    fired.add("lo")
                    c = prev + 1
                if c > prev + jm:
                    fired.add("hi")
                    c = prev + jm
                if nb - c < 8 - k:
                    fired.add("need_after")
                    c = nb - (8 - k)
                if nb - c > (8 - k) * jm:
                    fired.add("room_after")
                    c = nb - (8 - k) * jm
                prev = c
            assert prev == X.bounds(table)[7]
    assert fired == {"lo", "hi", "need_after", "room_after"}, fired


def test_fewer_than_8_blocks_break_the_rule():
    """Why balance mode is gated at 8 blocks: below, need_after (every later XCD needs a block) pushes a cut under the
    one before it.  With 7 blocks that is one empty range and nothing worse; with 6 or fewer the cuts go below 0, an XCD
    starts at a negative logical block, and the walk would read and write in front of its arrays."""
    assert X.MIN_BLOCKS == 8
    assert X.bounds(np.zeros((5, 4), dtype=np.uint32)) == [0, -2, -1, 0, 1, 2, 3, 4, 5]
    for nb in range(1, 8):
        jm = X.jmax(nb)
        for name, table in X.patterns(nb):
            b = X.bounds(table)
            assert min(np.diff(b)) < 1, (nb, name, b)  # "every range holds at least one block" fails at every nb < 8
            if nb <= 6:
                assert min(b) == nb - 7 < 0 and int(X.walked_blocks(b, jm).min()) < 0, (nb, name, b)
                assert not X.covers_once(b, nb, jm), (nb, name, b)
            else:
                assert min(b) == 0, (nb, name, b)


def test_covers_once_rejects_what_it_must():
    """The checker on hand-made bounds: 17 blocks, 5 workgroups per XCD."""
    nb, jm = 17, 5
    assert X.jmax(nb) == jm
    good = [0, 3, 5, 7, 9, 11, 13, 15, 17]
    assert X.bounds(np.zeros((nb, 4), dtype=np.uint32)) == good
    assert X.covers_once(good, nb, jm)
    assert X.covers_once([0, 3, 3, 7, 9, 11, 13, 15, 17], nb, jm)      # an empty range harms nothing by itself
    assert not X.covers_once([0, 3, 5, 7, 9, 11, 13, 15, 16], nb, jm)  # the last block is never walked
    assert not X.covers_once([1, 3, 5, 7, 9, 11, 13, 15, 17], nb, jm)  # nor the first
    assert not X.covers_once([0, 3, 5, 7, 9, 11, 13, 15, 18], nb, jm)  # a block beyond the end is walked
    assert not X.covers_once([0, 6, 7, 8, 9, 11, 13, 15, 17], nb, jm)  # 6 blocks, 5 workgroups: block 5 is dropped
    assert not X.covers_once([0, 3, 5, 4, 9, 11, 13, 15, 17], nb, jm)  # block 4 is walked by XCD 1 and by XCD 3
    assert not X.covers_once([0, 2, 5, 7, 9, 11, 13, 15, 17], nb, 2)   # the same launch too small for a range of 3
    assert not X.covers_once([0, -2, -1, 0, 1, 2, 3, 4, 5], 5, X.jmax(5))


def test_logical_block_is_a_permutation():
    for chunk in CHUNKS:
        for nb in range(1, 301):
            got = sorted(X.logical_block(b, nb, chunk) for b in range(nb))
            assert got == list(range(nb)), (chunk, nb)


def test_jmax_leaves_room():
    for nb in list(range(1, 5000)) + list(BIG):
        assert 8 * X.jmax(nb) >= nb + 8, nb  # every XCD can hold its eighth and at least one block more
