"""The keys-only radix sort (csrc/radix.hip, sort_keys) against NumPy through nbmi_debug_sort_keys: the output is the
input keys in the stable order of their bits [begin_bit, end_bit), whole words (the bits outside the field travel with
their key and decide nothing).  The octree build sorts (prefix << 24 | body index) words this way instead of
(key, index) pairs; the last test is the equivalence that rests on.  Exact equality everywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# wave, tile and multi-tile edges; both sides of the keys-per-thread switches (4 -> 8 at 65 536, 8 -> 16 at 524 288)
SIZES = [1, 2, 63, 64, 65, 4095, 4096, 4097, 12_289]
SWITCH_SIZES = [65_536, 65_537, 524_288, 524_289]
# [24, 64) and [24, 40) leave unsorted low bits, as the packed word has; for 32-bit keys the ranges end at bit 32
RANGES = [(0, 63), (0, 17), (24, 64), (24, 40)]


def _sort_keys(nat, keys, begin, end, repeats=1):
    out = np.empty_like(keys)
    ms = C.c_double(0.0)
    nat.check(nat.load().nbmi_debug_sort_keys(keys.dtype.itemsize, len(keys), nat.ptr(keys), nat.ptr(out), begin, end,
                                              repeats, C.addressof(ms)), "nbmi_debug_sort_keys")
    return out


def _cases(rng, n, dtype, bits):
    """The six key patterns of tests/test_gpu_sort.py, `bits` wide."""
    top = (1 << bits) - 1
    yield "uniform", rng.integers(0, top, n, dtype=np.uint64, endpoint=True).astype(dtype)
    yield "few distinct", (rng.integers(0, 5, n, dtype=np.uint64) * np.uint64(top // 7)).astype(dtype)
    yield "all equal", np.full(n, top // 3, dtype=dtype)
    yield "sorted", np.sort(rng.integers(0, top, n, dtype=np.uint64, endpoint=True)).astype(dtype)
    yield "reversed", np.sort(rng.integers(0, top, n, dtype=np.uint64, endpoint=True))[::-1].astype(dtype).copy()
    yield "shared upper digits", ((np.uint64(top) >> np.uint64(2)) ^ rng.integers(0, 1 << min(bits, 20), n, dtype=np.uint64)).astype(dtype)


def _expected(keys, begin, end):
    field = (keys.astype(np.uint64) >> np.uint64(begin)) & np.uint64((1 << (end - begin)) - 1)
    return keys[np.argsort(field, kind="stable")]


def _check_all(nat, n):
    rng = np.random.default_rng(n)
    for dtype in (np.uint64, np.uint32):
        width = 8 * np.dtype(dtype).itemsize
        # the patterns fill the whole word, so every range has bits below and / or above it that must not matter
        for name, keys in _cases(rng, n, dtype, width):
            for begin, end in RANGES:
                end = min(end, width)
                got = _sort_keys(nat, keys, begin, end)
                assert np.array_equal(got, _expected(keys, begin, end)), (name, np.dtype(dtype).name, begin, end)


@pytest.mark.parametrize("n", SIZES)
def test_sort_keys_matches_numpy(gpu, n):
    import nbmi_native as nat
    _check_all(nat, n)


@pytest.mark.parametrize("n", SWITCH_SIZES)
def test_sort_keys_at_tile_size_switches(gpu, n):
    import nbmi_native as nat
    _check_all(nat, n)


@pytest.mark.parametrize("n", [4097, 100_003])
def test_packed_word_sort_is_the_stable_pair_sort(gpu, n):
    """(prefix << 24 | index) sorted on [24, 64) = the indices in the stable order of the prefixes alone."""
    import nbmi_native as nat
    rng = np.random.default_rng(n)
    # heavily repeated 40-bit prefixes: 37 distinct values, spread over all five digits
    prefix = rng.integers(0, 1 << 40, 37, dtype=np.uint64)[rng.integers(0, 37, n)]
    packed = (prefix << np.uint64(24)) | np.arange(n, dtype=np.uint64)
    got = _sort_keys(nat, packed, 24, 64)
    order = np.argsort(prefix, kind="stable")
    assert np.array_equal(got & np.uint64((1 << 24) - 1), order.astype(np.uint64))
    assert np.array_equal(got >> np.uint64(24), prefix[order])


def test_sort_keys_refuses_bad_ranges(gpu):
    import nbmi_native as nat
    keys = np.arange(8, dtype=np.uint32)
    out = np.empty_like(keys)
    lib = nat.load()
    for begin, end in ((0, 33), (8, 8), (-1, 8), (9, 3)):
        assert lib.nbmi_debug_sort_keys(4, 8, nat.ptr(keys), nat.ptr(out), begin, end, 1, None) != 0, (begin, end)
