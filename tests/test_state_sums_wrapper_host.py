"""The helper behind deposit() and radial_profile() (nbody/gpu_backend.py, no device): for every subset of quantity
names its bits, its plane count and the layout of its result dict are what the two wrappers built by hand before."""
import ctypes as C
import itertools

import numpy as np
import pytest


def _by_hand(names_in, table, vector, shape, stats, extra):
    """the wrappers' own lines before the helper, with the planes filled as the stand-in call below fills them"""
    names = [q for q in table if q in names_in]
    bits = sum(table[q] for q in names)
    planes = sum(3 if q == vector else 1 for q in names)
    out = np.arange(planes * int(np.prod(shape)), dtype=np.float64).reshape((planes,) + shape)
    res, p = {}, 0
    for q in names:
        res[q] = out[p:p + 3] if q == vector else out[p]
        p += 3 if q == vector else 1
    res.update(extra)
    res["exponents"] = np.arange(planes, dtype=np.int32) - 7
    if stats:
        res["stats"] = (11, 12, 13)
    return bits, planes, res


@pytest.mark.parametrize("which", ["deposit", "radial_profile"])
def test_helper_matches_the_wrappers_by_hand(which):
    from nbody import gpu_backend as gb
    table, vector, shape, extra = {
        "deposit": (gb.DEPOSIT_QUANTITIES, "momentum", (2, 3, 4), {}),
        "radial_profile": (gb.PROFILE_QUANTITIES, "angular_momentum", (5,), {"center": "c", "bulk_velocity": "b"}),
    }[which]
    for k in range(1, len(table) + 1):
        for subset in itertools.combinations(reversed(list(table)), k):  # (given out of order: the table's order rules)
            for stats in (False, True):
                bits, planes, want = _by_hand(subset, table, vector, shape, stats, extra)
                seen = {}

                def call(b, out, st, ex):
                    seen["bits"] = b
                    n = planes * int(np.prod(shape))
                    C.cast(out, C.POINTER(C.c_double * n)).contents[:] = list(range(n))
                    C.cast(st, C.POINTER(C.c_int64 * 3)).contents[:] = [11, 12, 13]
                    C.cast(ex, C.POINTER(C.c_int32 * planes)).contents[:] = [p - 7 for p in range(planes)]

                names = gb._sum_names(which, subset, table)
                got = gb._sum_planes(names, table, vector, shape, stats, extra, call)
                assert seen["bits"] == bits
                assert list(got) == list(want)  # keys and their order
                for key in want:
                    if isinstance(want[key], np.ndarray):
                        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape
                        assert np.array_equal(got[key], want[key])
                    else:
                        assert got[key] == want[key]
    assert gb._sum_names(which, next(iter(table)), table) == [next(iter(table))]  # a single name as a string
    for bad in ((), ("mass", "nope")):
        with pytest.raises(ValueError, match=f"^{which}: quantities must be some of "):
            gb._sum_names(which, bad, table)
