"""Plain integer restatement of how the tree walk deals its logical blocks (256 consecutive ranks each) to the eight
XCDs (csrc/nbmi.hip: logical_block, xcd_jmax, k_xcd_bounds).  TEST INFRASTRUCTURE ONLY.
Everything here is exact: Python integers or uint64 sums that cannot overflow (4 nb words of 32 bits).

    jmax(nb)                     workgroups per XCD of a balanced launch
    weights(table)               per block: its 4 wave times + 1
    raw_cuts(table)              the seven cuts before the clamps, by np.searchsorted on the prefix sums
    raw_cuts_loop(table)         the same by the kernel's own route: 1 024 threads, a chunk each, a scan, a loop
    clamp(cuts, nb, jm)          the four clamps in the kernel's order -> the 9 bounds
    bounds(table)                clamp(raw_cuts(table))
    covers_once(bounds, nb, jm)  the property the walk needs; knows nothing of the clamps
    logical_block(b, nb, chunk)  the mapping of the walks that are not in balance mode
    patterns(nb)                 the tables of wave times every test of the cut uses

A table is a (nb, 4) uint32 array: row i holds how long the four waves of logical block i took.
"""
import numpy as np

XCDS = 8
MIN_BLOCKS = 8          # below this no XCD range can hold "at least one block": the kernel's precondition
THREADS = 1024          # of the cut kernel's one workgroup
FULL = 0xFFFFFFFF


def jmax(nb):
    return ((nb + 7) // 8) * 3 // 2 + 1


def weights(table):
    t = np.asarray(table)
    assert t.dtype == np.uint32 and t.ndim == 2 and t.shape[1] == 4, (t.dtype, t.shape)
    return t.astype(np.uint64).sum(axis=1) + np.uint64(1)


def raw_cuts(table):
    """cut_k = min((first i with pre[i + 1] > target_k) + 1, nb), target_k = total // 8 * k, for k = 1 .. 7."""
    w = weights(table)
    nb = len(w)
    inc = np.cumsum(w, dtype=np.uint64)  # inc[i] = pre[i + 1]
    total = int(inc[-1])
    out = []
    for k in range(1, XCDS):
        target = total // 8 * k
        i = int(np.searchsorted(inc, np.uint64(target), side="right"))  # the first i with inc[i] > target
        out.append(min(i + 1, nb))
    return out


def raw_cuts_loop(table):
    """The kernel's route, literally: thread t sums the blocks [t chunk, (t + 1) chunk), the sums are scanned, and a
    thread whose chunk holds target_k (ex <= target_k < inc) adds its blocks up again until it passes it."""
    w = [int(x) for x in weights(table)]
    nb = len(w)
    chunk = (nb + THREADS - 1) // THREADS
    span = [(min(t * chunk, nb), min(min(t * chunk, nb) + chunk, nb)) for t in range(THREADS)]
    acc = [sum(w[b:e]) for b, e in span]
    ex, run = [], 0
    for a in acc:
        ex.append(run)
        run += a
    total = run
    cut = {}
    for k in range(1, XCDS):
        target = total // 8 * k
        for t, (b, e) in enumerate(span):
            if b < e and ex[t] <= target < ex[t] + acc[t]:
                run, i = ex[t], b
                while i < e:
                    run += w[i]
                    if run > target:
                        break
                    i += 1
                assert k not in cut, "two threads claim one cut"
                cut[k] = min(i + 1, nb)
    assert sorted(cut) == list(range(1, XCDS)), "a cut that no thread writes"
    return [cut[k] for k in range(1, XCDS)]


def clamp(cuts, nb, jm):
    """Ranges of 1 .. jm blocks in order; what a clamp pushes out goes to the later XCDs."""
    b = [0]
    prev = 0
    for k in range(1, XCDS):
        c = cuts[k - 1]
        lo, hi = prev + 1, prev + jm
        need_after = XCDS - k
        room_after = (XCDS - k) * jm
        if c < lo:
            c = lo
        if c > hi:
            c = hi
        if nb - c < need_after:
            c = nb - need_after
        if nb - c > room_after:
            c = nb - room_after
        b.append(c)
        prev = c
    b.append(nb)
    return b


def bounds(table):
    nb = len(table)
    return clamp(raw_cuts(table), nb, jmax(nb))


def walked_blocks(b, jm):
    """The logical blocks a balanced launch of 8 jm workgroups walks, in workgroup order: workgroup (xcd, jb) takes
    b[xcd] + jb if that is below b[xcd + 1], and nothing otherwise."""
    assert len(b) == XCDS + 1
    parts = [np.arange(int(b[x]), min(int(b[x + 1]), int(b[x]) + jm), dtype=np.int64) for x in range(XCDS)]
    return np.concatenate(parts)


def covers_once(b, nb, jm):
    got = walked_blocks(b, jm)
    return len(got) == nb and np.array_equal(np.sort(got), np.arange(nb, dtype=np.int64))


def logical_block(b, nb, chunk):
    """chunk < 0: identity; 0: one contiguous eighth per XCD; > 0: runs of `chunk` blocks dealt round over the XCDs,
    the blocks behind the last complete round of 8 chunks as they come."""
    if chunk < 0:
        return b
    xcd, j = b & 7, b >> 3
    if chunk == 0:
        q, rem = nb >> 3, nb & 7
        return xcd * q + min(xcd, rem) + j
    span = 8 * chunk
    full = (nb // span) * span
    if b >= full:
        return b
    return ((j // chunk) * 8 + xcd) * chunk + (j % chunk)


def patterns(nb):
    """(name, table) pairs: flat, saturated, one hot block, a hot eighth at either end, monotone, random."""
    def flat(v):
        return np.full((nb, 4), v, dtype=np.uint32)

    def hot(lo, hi):
        t = flat(1000)
        t[lo:hi] = FULL
        return t

    eighth = max(nb // 8, 1)
    ramp = (16 * np.arange(nb, dtype=np.uint64)[:, None] + np.arange(4, dtype=np.uint64)[None, :]).astype(np.uint32)
    out = [("zero", flat(0)), ("full", flat(FULL)),
           ("hot_first", hot(0, 1)), ("hot_middle", hot(nb // 2, nb // 2 + 1)), ("hot_last", hot(nb - 1, nb)),
           ("front_heavy", hot(0, eighth)), ("back_heavy", hot(nb - eighth, nb)),
           ("increasing", ramp), ("decreasing", np.ascontiguousarray(ramp[::-1]))]
    for seed in (1, 2, 3):
        rng = np.random.default_rng(1000 * seed + 7)
        if seed == 1:    # the whole range of a word
            t = rng.integers(0, 2 ** 32, (nb, 4), dtype=np.uint64)
        elif seed == 2:  # close to one another, as a relaxed system's waves are
            t = rng.integers(50_000, 60_000, (nb, 4), dtype=np.uint64)
        else:            # over nine decades: a few blocks carry nearly everything
            t = np.exp(rng.uniform(0.0, np.log(2.0 ** 32 - 1), (nb, 4))).astype(np.uint64)
        out.append((f"random{seed}", t.astype(np.uint32)))
    for _, t in out:
        assert t.shape == (nb, 4) and t.dtype == np.uint32 and t.flags.c_contiguous
    return out
