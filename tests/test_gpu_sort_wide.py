"""The radix sort's pass configurations (csrc/radix.hip: digit width 8 or 10 bits, 256 / 512 / 1024 threads on a
4 096-key tile) against NumPy through nbmi_debug_sort_config, which reaches with small inputs what the size rule keeps
for large ones.  Every configuration must give keys[np.argsort(field, kind="stable")] exactly: whole words, the bits
outside the field travelling along.  All six combinations are covered: the shipped ones (8 bits x 256; for keys-only
sorts of more than 524 288 keys 10 bits x 1024, and 8 bits x 512 above 2 097 152) and the ones only the switches reach.

The hooks keep one temp buffer per process, so successive calls here - other sizes, fields and configurations - also
check that each sort clears what the one before left in it.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONFIGS = [(b, t) for b in (8, 10) for t in (256, 512, 1024)]
# tile edges, more than one look-back batch of tiles (40 961 = 11 tiles), 74 tiles
SIZES = [1, 4095, 4096, 4097, 8193, 40_961, 300_001]
# the product's field (four whole 10-bit digits), a partial last digit, one pass, a field in the middle of the word
FIELDS = [(24, 64), (24, 57), (0, 10), (3, 40)]


def _sort(nat, keys, begin, end, bits, threads, repeats=1, values=None):
    out = np.empty_like(keys)
    vout = None if values is None else np.empty_like(values)
    ms = C.c_double(0.0)
    nat.check(nat.load().nbmi_debug_sort_config(keys.dtype.itemsize, len(keys), nat.ptr(keys),
                                                None if values is None else nat.ptr(values), nat.ptr(out),
                                                None if values is None else nat.ptr(vout), begin, end, bits, threads,
                                                repeats, C.addressof(ms)), "nbmi_debug_sort_config")
    return out if values is None else (out, vout)


def _field(keys, begin, end):
    return (keys.astype(np.uint64) >> np.uint64(begin)) & np.uint64((1 << (end - begin)) - 1)


def _expected(keys, begin, end):
    return keys[np.argsort(_field(keys, begin, end), kind="stable")]


def _with_field(rng, field, begin, end):
    """64-bit words whose bits [begin, end) are `field`: the row index below the field, random bits above it."""
    n = len(field)
    low = np.arange(n, dtype=np.uint64) & np.uint64((1 << begin) - 1)
    high = rng.integers(0, 1 << (64 - end), n, dtype=np.uint64) << np.uint64(end) if end < 64 else np.uint64(0)
    return (field << np.uint64(begin)) | low | high


def _inputs(rng, n, begin, end):
    width = end - begin
    top = (1 << width) - 1
    rand = rng.integers(0, top, n, dtype=np.uint64, endpoint=True)
    yield "random", _with_field(rng, rand, begin, end)
    yield "sorted", _with_field(rng, np.sort(rand), begin, end)
    yield "reversed", _with_field(rng, np.sort(rand)[::-1].copy(), begin, end)
    # one bin takes the whole tile in every pass: the per-wave counters reach their largest value
    yield "all equal", _with_field(rng, np.full(n, (top // 3) | 1, dtype=np.uint64), begin, end)
    two = np.array([top // 5, top - top // 7], dtype=np.uint64)
    yield "two values", _with_field(rng, two[rng.integers(0, 2, n)], begin, end)
    # the octree build's words: the state is kept in last step's order, so the upper digits arrive sorted and only the
    # lowest digit is random
    lowbits = min(10, width)
    upper = np.sort(rng.integers(0, 1 << (width - lowbits), n, dtype=np.uint64)) if width > lowbits else np.zeros(n, np.uint64)
    yield "product", _with_field(rng, (upper << np.uint64(lowbits)) | rng.integers(0, 1 << lowbits, n, dtype=np.uint64), begin, end)


@pytest.mark.parametrize("n", SIZES)
def test_every_configuration_matches_numpy(gpu, n):
    import nbmi_native as nat
    rng = np.random.default_rng(n)
    for begin, end in FIELDS:
        for name, keys in _inputs(rng, n, begin, end):
            want = _expected(keys, begin, end)
            for bits, threads in CONFIGS:
                got = _sort(nat, keys, begin, end, bits, threads)
                assert np.array_equal(got, want), (name, begin, end, bits, threads)


def test_size_rule_matches_numpy(gpu):
    """digit_bits = threads = 0: what the sort chooses itself, on both sides of the sizes at which it changes its mind
    (8 bits x 256 up to 524 288 keys, 10 bits x 1024 up to 2 097 152 where the field suits them, 8 bits x 512 beyond)."""
    import nbmi_native as nat
    for n in (524_288, 524_289, 2_097_152, 2_097_153):
        rng = np.random.default_rng(n)
        for begin, end in ((24, 64), (24, 57)) if n < 1_000_000 else ((24, 64),):
            keys = rng.integers(0, (1 << 64) - 1, n, dtype=np.uint64, endpoint=True)
            assert np.array_equal(_sort(nat, keys, begin, end, 0, 0), _expected(keys, begin, end)), (n, begin, end)


@pytest.mark.parametrize("bits,threads", CONFIGS)
def test_repeated_sorts_on_one_temp_buffer(gpu, bits, threads):
    """Different n and fields one after the other, each run three times (repeats = 2 after the untimed first run): a sort
    finds the tickets, histogram and status rows of the previous one - a larger sort with more passes and a smaller
    one with fewer - and must have cleared all that it uses."""
    import nbmi_native as nat
    rng = np.random.default_rng(bits * threads)
    for n, (begin, end) in ((40_961, (24, 64)), (4097, (0, 10)), (8193, (3, 40)), (300_001, (24, 57)), (4095, (24, 64))):
        keys = rng.integers(0, (1 << 64) - 1, n, dtype=np.uint64, endpoint=True)
        got = _sort(nat, keys, begin, end, bits, threads, repeats=2)
        assert np.array_equal(got, _expected(keys, begin, end)), (n, begin, end)


@pytest.mark.parametrize("bits,threads", CONFIGS)
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_pairs_in_every_configuration(gpu, bits, threads, dtype):
    """The pair form of the same templates: (key, value) by the key's bits, stable."""
    import nbmi_native as nat
    width = 8 * np.dtype(dtype).itemsize
    for n in (4097, 40_961):
        rng = np.random.default_rng(n + bits + threads)
        keys = rng.integers(0, (1 << width) - 1, n, dtype=np.uint64, endpoint=True).astype(dtype)
        keys[n // 2:] = keys[:n - n // 2]  # equal keys far apart: stability shows in the values
        vals = np.arange(n, dtype=np.uint32)
        for begin, end in ((0, 24), (5, width - 1)):
            order = np.argsort(_field(keys, begin, end), kind="stable")
            ko, vo = _sort(nat, keys, begin, end, bits, threads, values=vals)
            assert np.array_equal(ko, keys[order]) and np.array_equal(vo, vals[order]), (n, begin, end)


def test_refuses_bad_arguments_before_launching(gpu):
    import nbmi_native as nat
    lib = nat.load()
    keys = np.arange(8, dtype=np.uint64)
    vals = np.arange(8, dtype=np.uint32)
    out = np.full(8, 0xdead, dtype=np.uint64)
    vout = np.empty(8, dtype=np.uint32)
    k, o, v, vo = nat.ptr(keys), nat.ptr(out), nat.ptr(vals), nat.ptr(vout)

    def call(key_bytes=8, n=8, keys=k, values=None, out=o, vout=None, begin=0, end=40, bits=10, threads=1024):
        return lib.nbmi_debug_sort_config(key_bytes, n, keys, values, out, vout, begin, end, bits, threads, 1, None)

    assert call() == 0 and np.array_equal(out, keys)
    out[:] = 0xdead
    for bad in (dict(bits=9), dict(bits=12), dict(bits=-8), dict(bits=1), dict(threads=128), dict(threads=64), dict(threads=2048),
                dict(threads=-256), dict(threads=300), dict(begin=-1), dict(begin=40, end=40), dict(begin=9, end=3), dict(end=65),
                dict(key_bytes=4, end=33), dict(key_bytes=2), dict(n=-1), dict(keys=None), dict(out=None),
                dict(values=v, vout=None)):
        assert call(**bad) != 0, bad
        assert np.all(out == 0xdead), bad  # nothing ran
    assert call(values=v, vout=vo, bits=0, threads=0) == 0 and np.array_equal(out, keys) and np.array_equal(vout, vals)
