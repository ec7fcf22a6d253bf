"""Systems, edges and raw-call helpers shared by tests/test_profile_host.py and tests/test_gpu_profile.py (include/nbmi.h
nbmi_radial_profile, nbmi_mass_radii).  Not a test module."""
import numpy as np

import profile_ref as pr

# sizes around a wave, around the 2 048 rows a workgroup of k_profile covers (which is also the scan tile of
# nbmi_mass_radii), around the 1 024 pairs of a sort tile at these sizes, around two of each, and one larger
SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 10_000]
CENTER = (1.0, -2.0, 3.0)  # small integers: axis-aligned integer offsets give r2 == E[k] exactly
BULK = (0.25, -0.5, 0.125)
FRACTIONS = (0.5, 0.1, 0.9, 0.25, 0.5, 1.0, 1e-9, 0.75)  # unsorted, one repeated, f = 1, one that gives T = 1


def cloud(n, seed=1, scale=2.0):
    """n bodies about CENTER: normal positions of width ``scale``, velocities with BULK added, masses in [0.5, 2)"""
    rng = np.random.RandomState(seed)
    p = rng.normal(size=(n, 3)) * scale + np.array(CENTER)
    v = rng.normal(size=(n, 3)) * 3.0 + np.array(BULK)
    return p, v, rng.uniform(0.5, 2.0, n)


def edges_for(nb, first=0.25, last=6.0):
    """nb + 1 edges from ``first`` (0 allowed) to ``last``, log-spaced above the first"""
    if nb == 1:
        return np.array([first, last])
    inner = np.geomspace(first if first > 0 else last / 2.0 ** 10, last, nb + 1)
    inner[0] = first
    return inner


def on_edges(edges):
    """Bodies exactly on every edge - offsets of +-edge along one axis from CENTER, so that r2 == E[k] in float64 when
    the edges are small integers or dyadic - one exactly at the centre, and one just outside each edge."""
    rows = [np.array(CENTER)]
    for k, e in enumerate(edges):
        d = np.zeros(3)
        d[k % 3] = e if k % 2 == 0 else -e
        rows.append(np.array(CENTER) + d)
        d2 = np.zeros(3)
        d2[(k + 1) % 3] = e + 2.0 ** -20  # (an offset that survives the sum with CENTER)
        rows.append(np.array(CENTER) + d2)
    return np.array(rows)


def handle(kind, p, v, m, **kw):
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation
    p, v, m = (np.ascontiguousarray(a, np.float64) for a in (p, v, m))
    if kind == "direct":
        return HIPDirectSimulation(p, v, m, 0.07, 1.5, 1.0, **kw)
    return HIPBarnesHutSimulation(p, v, m, 0.07, 1.5, 1.0, 0.5, **kw)


class Handles:
    """the handle of a case as a list of one (a measurement knob with two forms would put two here), closed on exit"""
    def __init__(self, p, v, m, kind="bh", **kw):
        self.sims = [handle(kind, p, v, m, **kw)]

    def __enter__(self):
        return self.sims

    def __exit__(self, *exc):
        for s in self.sims:
            s.close()


PROFILE_FILL, INT_FILL = -3.5, -7


def raw_profile(nat, sim, center, bulk, edges, quantities, nb=None):
    """the C call itself: (rc, out (P, nb + 1), stats3, exponents); the outputs hold fill values beforehand"""
    e = np.array(edges, dtype=np.float64)
    nb = len(e) - 1 if nb is None else nb
    planes = len(pr.planes_of(quantities)) if 0 < quantities < 64 else 1
    out = np.full((planes, max(len(e), 1)), PROFILE_FILL, dtype=np.float64)
    st, ex = np.full(3, INT_FILL, dtype=np.int64), np.full(planes, INT_FILL, dtype=np.int32)
    c = None if center is None else np.array(center, dtype=np.float64)
    b = None if bulk is None else np.array(bulk, dtype=np.float64)
    rc = nat.load().nbmi_radial_profile(sim._h, nat.ptr(c), nat.ptr(b), int(nb), nat.ptr(e), int(quantities), nat.ptr(out),
                                        nat.ptr(st), nat.ptr(ex))
    return rc, out, st, ex


def raw_radii(nat, sim, center, fractions, nf=None):
    """the C call itself: (rc, radius2, inside, mass_inside, total_mass, stats2, exponent), fill values beforehand"""
    import ctypes as C
    f = np.array(fractions, dtype=np.float64)
    nf = len(f) if nf is None else nf
    r2 = np.full(max(len(f), 1), PROFILE_FILL)
    ins = np.full(max(len(f), 1), INT_FILL, dtype=np.int64)
    mass = np.full(max(len(f), 1), PROFILE_FILL)
    total, ex = C.c_double(PROFILE_FILL), C.c_int32(INT_FILL)
    st = np.full(2, INT_FILL, dtype=np.int64)
    c = None if center is None else np.array(center, dtype=np.float64)
    rc = nat.load().nbmi_mass_radii(sim._h, nat.ptr(c), int(nf), nat.ptr(f), nat.ptr(r2), nat.ptr(ins), nat.ptr(mass),
                                    C.addressof(total), nat.ptr(st), C.addressof(ex))
    return rc, r2, ins, mass, float(total.value), st, int(ex.value)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def radii_untouched(got):
    rc, r2, ins, mass, total, st, ex = got
    return ((r2 == PROFILE_FILL).all() and (ins == INT_FILL).all() and (mass == PROFILE_FILL).all() and total == PROFILE_FILL
            and (st == INT_FILL).all() and ex == INT_FILL)
