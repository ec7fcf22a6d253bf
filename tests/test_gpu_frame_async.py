"""Asynchronous frame fetch (nbmi_frame_begin / _wait / _release / _pending) and the recorder's opt-in
pipelined loop, on the device: the same bits as the synchronous calls, snapshots that later steps do not touch, slot
discipline, no influence on the simulation, deferred errors, and record(pipeline=True) == record() file by file."""
import io
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bodies(n, seed=3):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)) * 50.0, rng.normal(size=(n, 3)) * 6.0, rng.uniform(0.5, 1.5, n)


def _make(method, integrator, pos, vel, mass, G=1.0, eps=0.5):
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation
    if method == "direct":
        return HIPDirectSimulation(pos, vel, mass, G, eps, 1.0, integrator=integrator)
    return HIPBarnesHutSimulation(pos, vel, mass, G, eps, 1.0, 0.5, integrator=integrator)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _need_zstd(rec):
    try:
        rec._load_zstd()
    except RuntimeError:
        pytest.skip("no libzstd")


# ---- 1. the same bits as the synchronous calls -----------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
@pytest.mark.parametrize("method", ["barnes_hut", "direct"])
@pytest.mark.parametrize("n", [1, 63, 2_000, 100_000])
def test_async_frames_are_the_synchronous_frames_bit_for_bit(gpu, n, method, integrator):
    pos, vel, mass = _bodies(n)
    a = _make(method, integrator, pos, vel, mass)  # asynchronous calls
    b = _make(method, integrator, pos, vel, mass)  # its twin: synchronous calls
    dt, sub = 0.05, (1 if n > 10_000 else 2)
    for s in (a, b):
        s.step_many(dt, sub)
    slot = a.frame_begin("f32", 15.0)
    p, c = a.frame_wait(slot)
    assert not p.flags.writeable and not c.flags.writeable and p.shape == c.shape == (n, 3)
    b.compute_colors(15.0)
    assert _same(p, b.get_positions()) and _same(c, b.get_colors())
    assert _same(a.get_colors(), c)  # the snapshot left compute_colors' result behind
    assert _same(a.get_positions(), p)
    a.frame_release(slot)

    slot = a.frame_begin("key", 15.0)
    p, c = a.frame_wait(slot)
    b.compute_colors(15.0)
    kp, kc = b.frame_keyframe()
    assert _same(p, kp) and _same(c, kc)
    a.frame_release(slot)
    wrapped = False
    for k in range(6):
        if k == 3:  # a jump of > 32.767 for some bodies: the int16 cast wraps (the forced wrap of the codec test)
            for s in (a, b):
                x, v = s.get_positions_f64(), s.get_velocities()
                x[::7] += [40.0, -70.0, 33.0]
                s.set_state(x, v)
        for s in (a, b):
            s.step_many(dt, sub)
        before = b.get_positions()
        slot = a.frame_begin("delta", 15.0)
        dp, dc = a.frame_wait(slot)
        b.compute_colors(15.0)
        sp, sc = b.frame_delta()
        assert dp.dtype == np.int16 and _same(dp, sp) and _same(dc, sc), k
        assert _same(a.get_colors(), b.get_colors()), k
        a.frame_release(slot)
        if k == 3:
            wrapped = bool((np.abs(before - kp) > 32.767).any())
    assert wrapped
    # mixed use: the chain is the order of the calls, whichever kind of call made them
    for s in (a, b):
        s.step_many(dt, sub)
    a.compute_colors(15.0)
    b.compute_colors(15.0)
    assert all(_same(x, y) for x, y in zip(a.frame_delta(), b.frame_delta()))
    for s in (a, b):
        s.step_many(dt, sub)
    slot = a.frame_begin("delta", 15.0)
    b.compute_colors(15.0)
    assert all(_same(x, y) for x, y in zip(a.frame_wait(slot), b.frame_delta()))
    a.frame_release(slot)
    assert _same(a.get_positions_f64(), b.get_positions_f64()) and _same(a.get_velocities(), b.get_velocities())
    a.close()
    b.close()


# ---- 2. a snapshot is a snapshot ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "key"])
def test_a_frame_is_the_state_at_its_begin(gpu, kind):
    pos, vel, mass = _bodies(50_000, seed=4)
    a = _make("barnes_hut", "kick_drift", pos, vel, mass)
    b = _make("barnes_hut", "kick_drift", pos, vel, mass)
    dt = 0.05
    want = []
    for s in (a, b):
        s.step_many(dt, 2)
    b.compute_colors(15.0)
    want.append((b.get_positions(), b.get_colors()))
    s0 = a.frame_begin(kind, 15.0)
    for _ in range(3):
        a.step_many(dt, 1)
    b.step_many(dt, 3)
    b.compute_colors(15.0)
    want.append((b.get_positions(), b.get_colors()))
    s1 = a.frame_begin("f32", 15.0)  # two frames in flight
    a.step_many(dt, 4)
    assert a.frames_pending() == [(s0, kind, 2), (s1, "f32", 5)] and a.step_count() == 9
    p1, c1 = a.frame_wait(s1)
    p0, c0 = a.frame_wait(s0)
    assert _same(p0, want[0][0]) and _same(c0, want[0][1])
    assert _same(p1, want[1][0]) and _same(c1, want[1][1])
    assert not np.array_equal(p0, p1)
    a.sync()
    assert _same(p0, want[0][0]) and _same(p1, want[1][0])  # still, after everything enqueued since has run
    b.step_many(dt, 4)
    assert _same(a.get_positions_f64(), b.get_positions_f64())
    a.frame_release(s0)
    a.frame_release(s1)
    a.close()
    b.close()


# ---- 3. slot discipline --------------------------------------------------------------------------------------------------
def test_slot_discipline(gpu):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    pos, vel, mass = _bodies(3_000, seed=5)
    a = _make("barnes_hut", "kick_drift", pos, vel, mass)
    assert a.frames_pending() == []
    with pytest.raises(ValueError, match="no previous frame"):
        a.frame_begin("delta")
    with pytest.raises(ValueError):
        a.frame_begin("jpeg")
    for slot in (0, 1, 2, -1):
        with pytest.raises(ValueError, match="holds no frame"):
            a.frame_wait(slot)
        with pytest.raises(ValueError, match="holds no frame"):
            a.frame_release(slot)
    a.step_many(0.05, 2)
    s0 = a.frame_begin("f32", 15.0)
    a.step_many(0.05, 3)
    s1 = a.frame_begin("key", 15.0)
    assert {s0, s1} == {0, 1}
    held = [tuple(x.copy() for x in a.frame_wait(s)) for s in (s0, s1)]
    colors = a.get_colors()
    a.step_many(0.05, 1)
    with pytest.raises(ValueError, match="no free frame slot"):
        a.frame_begin("f32", 3.0)
    # ... and it changed nothing: the slots, their payloads, the colours, the step count
    assert a.frames_pending() == [(s0, "f32", 2), (s1, "key", 5)] and a.step_count() == 6
    assert _same(a.get_colors(), colors)
    for s, h in zip((s0, s1), held):
        assert all(_same(x, y) for x, y in zip(a.frame_wait(s), h))  # waiting twice is allowed
    a.frame_release(s0)
    with pytest.raises(ValueError, match="holds no frame"):
        a.frame_release(s0)
    with pytest.raises(ValueError, match="holds no frame"):
        a.frame_wait(s0)
    s2 = a.frame_begin("delta", 15.0)  # the key frame above is the previous frame
    assert s2 == s0 and a.frames_pending() == [(s1, "key", 5), (s2, "delta", 6)]  # begin order, not slot order
    a.frame_release(s1)
    a.frame_release(s2)  # released without a wait: the next begin on this slot is ordered behind its copy
    s3 = a.frame_begin("f32", 15.0)
    p, _ = a.frame_wait(s3)
    assert _same(p, a.get_positions())
    a.frame_release(s3)
    assert a.frames_pending() == []
    a.close()
    # n == 0: empty payloads of the right type
    z = HIPBarnesHutSimulation(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), 1.0, 0.5, 1.0, 0.5)
    for kind, dtype in (("f32", np.float32), ("key", np.float32)):
        s = z.frame_begin(kind)
        p, c = z.frame_wait(s)
        assert p.shape == c.shape == (0, 3) and p.dtype == c.dtype == dtype
        assert z.frames_pending() == [(s, kind, 0)]
        z.frame_release(s)
    z.close()


# ---- 4. frames do not change the simulation -----------------------------------------------------------------------------
def test_non_interference_1m(gpu):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    res = []
    for frames in (False, True):
        s = HIPBarnesHutSimulation.generated("galaxy", 1_000_000, 500.0, 0.15, 3.0, 1.0, 0.5, seed=7)
        prev = None
        for k in range(60):
            s.step(0.25)
            if frames:
                slot = s.frame_begin(("f32", "key", "delta")[min(k, 2)] if k % 2 else "f32", 15.0)
                if prev is not None:
                    s.frame_wait(prev)
                    s.frame_release(prev)
                prev = slot
        if prev is not None:
            s.frame_wait(prev)
            s.frame_release(prev)
        res.append((s.get_positions_f64(), s.get_velocities(), s.step_count(), s.force_precision_share()))
        s.close()
    a, b = res
    print("precision share and all-float64 flag at the end:", a[3])
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    assert a[2] == b[2] == 60 and a[3] == b[3]


# ---- 5. deferred errors --------------------------------------------------------------------------------------------------
def test_capacity_error_is_reported_by_the_frame_taken_after_it(gpu):
    """The octree overflow of test_capacity_error_in_the_middle_of_step_many_is_sticky: pairs meet to within 1e-9 after
    exactly one step, and the build of the second step needs more rows than there are.  A handled error code."""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    n_pairs, dt, sep = 1500, 0.1, 1.0
    rng = np.random.RandomState(7)
    base = rng.uniform(-50, 50, (n_pairs, 3))
    pos = np.concatenate([base, base + [sep, 0.0, 0.0]])
    v = (sep - 1e-9) / (2 * dt)
    vel = np.concatenate([np.tile([v, 0.0, 0.0], (n_pairs, 1)), np.tile([-v, 0.0, 0.0], (n_pairs, 1))])
    sim = HIPBarnesHutSimulation(pos, vel, np.ones(2 * n_pairs), 0.0, 0.1, 1.0, 0.5)
    sim.step_many(dt, 1)
    good = sim.frame_begin("f32", 15.0)  # before the failing step
    sim.step_many(dt, 2)
    bad = sim.frame_begin("f32", 15.0)   # after it
    p, _ = sim.frame_wait(good)
    assert _same(p, (pos + vel * dt).astype(np.float32))
    with pytest.raises(RuntimeError, match=r"code -4.*octree needs"):
        sim.frame_wait(bad)
    with pytest.raises(RuntimeError, match=r"code -4.*octree needs"):
        sim.frame_wait(bad)  # not cleared by the wait
    assert sim.frames_pending() == [(good, "f32", 1), (bad, "f32", 3)]
    sim.frame_release(good)
    sim.frame_release(bad)
    with pytest.raises(RuntimeError, match="octree needs"):
        sim.sync()  # still reported here, once
    sim.sync()
    assert np.array_equal(sim.get_positions_f64(), pos + vel * dt)  # the state of the last completed step
    late = sim.frame_begin("f32", 15.0)  # the words are clear again
    p, _ = sim.frame_wait(late)
    assert _same(p, (pos + vel * dt).astype(np.float32))
    sim.frame_release(late)
    sim.close()


# ---- 6. record(pipeline=True) writes the files record() writes -----------------------------------------------------
def _config(**kw):
    from tools.presets import get_preset_config
    cfg = get_preset_config("quick_galaxy")
    cfg.update(num_bodies=2000, theta=0.5)
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("zstd", [False, True])
def test_pipelined_recording_is_the_sequential_recording(gpu, tmp_path, zstd):
    from tools import record as rec
    if zstd:
        _need_zstd(rec)
    cfg = _config(total_frames=63, substeps=2, zstd=zstd, diagnostics_every=4 if zstd else 5)
    seq = rec.record(dict(cfg, session_name="seq"), root=tmp_path, quiet=True, seed=5)
    pipe = rec.record(dict(cfg, session_name="pipe", pipeline=True), root=tmp_path, quiet=True, seed=5)
    names = sorted(p.name for p in seq.iterdir())
    assert names == sorted(p.name for p in pipe.iterdir())
    ext = "zstd" if zstd else "npz"
    assert [n for n in names if n.startswith("frame_")] == [f"frame_{k:04d}.{ext}" for k in range(63)]
    assert [n for n in names if n.startswith("state_")] == ["state_0049.npz"]
    for name in names:
        if name.startswith(("frame_", "state_")):
            assert (seq / name).read_bytes() == (pipe / name).read_bytes(), name
    a = (seq / rec.DIAGNOSTICS_FILE).read_text().splitlines()
    b = (pipe / rec.DIAGNOSTICS_FILE).read_text().splitlines()
    assert a == b and len(a) == 1 + 63 // (4 if zstd else 5)
    ma, mb = rec.load_metadata(seq), rec.load_metadata(pipe)
    assert mb.pop("pipeline") is True and "pipeline" not in ma
    for m in (ma, mb):
        for key in ("start_time", "start_datetime", "session_name"):
            m.pop(key, None)
    assert ma == mb
    # extend picks the key up from metadata.json and continues the same files
    rec.extend_recording("pipe", 5, root=tmp_path)
    rec.extend_recording("seq", 5, root=tmp_path)
    assert rec.load_metadata(pipe)["pipeline"] is True and rec.get_completed_frames(pipe) == 68
    for k in range(68):
        a, _ = rec.load_frame(pipe, k)
        b, _ = rec.load_frame(seq, k)
        assert np.abs(a - b).max() <= (4e-3 if zstd else 1e-5), k


# ---- 7. interrupts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zstd", [False, True])
@pytest.mark.parametrize("point", ["after_step", "after_begin", "after_write", "in_atomically"])
def test_interrupted_pipelined_recording_resumes_to_the_uninterrupted_one(gpu, tmp_path, monkeypatch, zstd, point):
    """The situations of the sequential recorder's interrupt tests (Ctrl-C delivered when the step call returns, after a
    frame write, inside _atomically) plus one right after frame_begin, with their tolerances.  In a .zstd recording the
    frame whose write was cut short comes back as a delta frame with the uninterrupted run's bytes."""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    from tools import record as rec
    if zstd:
        _need_zstd(rec)
    total, substeps = 9, 3
    cfg = _config(total_frames=total, substeps=substeps, zstd=zstd, pipeline=True)
    whole = rec.record(dict({k: v for k, v in cfg.items() if k != "pipeline"}, session_name="whole"), root=tmp_path,
                       quiet=True, seed=11)
    calls = {"n": 0}

    def after(real, nth):
        def f(*a, **k):
            out = real(*a, **k)
            calls["n"] += 1
            if calls["n"] == nth:
                raise KeyboardInterrupt
            return out
        return f

    real_atomically = rec._atomically
    if point == "after_step":      # frame 4 has been stepped on the device, it has no slot; frame 3 is in flight
        monkeypatch.setattr(HIPBarnesHutSimulation, "step_many", after(HIPBarnesHutSimulation.step_many, 5))
        at, cut_frame = 4, 3
    elif point == "after_begin":   # frame 4 has its slot, the loop has not stored it; frame 3 is in flight
        monkeypatch.setattr(HIPBarnesHutSimulation, "frame_begin", after(HIPBarnesHutSimulation.frame_begin, 5))
        at, cut_frame = 4, 3
    elif point == "after_write":   # frame 3 is on disk and not released; frame 4 is in flight
        name = "write_bytes_atomic" if zstd else "save_frame"
        monkeypatch.setattr(rec, name, after(getattr(rec, name), 4))
        at, cut_frame = 4, 4
    else:                          # half of frame 3's bytes are written, then the interrupt arrives; frame 4 is in flight
        def cut_short(path, write):
            if path.name.startswith("frame_"):
                calls["n"] += 1
                if calls["n"] == 4:
                    def half(f):
                        buf = io.BytesIO()
                        write(buf)
                        f.write(buf.getvalue()[: len(buf.getvalue()) // 2])
                        f.flush()
                        raise KeyboardInterrupt
                    return real_atomically(path, half)
            return real_atomically(path, write)
        monkeypatch.setattr(rec, "_atomically", cut_short)
        at, cut_frame = 4, 3
    with pytest.raises(KeyboardInterrupt):
        rec.record(dict(cfg, session_name="cut"), root=tmp_path, quiet=True, seed=11)
    monkeypatch.undo()
    cut = tmp_path / "recordings" / "cut"
    assert not list(cut.glob(".*.part")), "a partial file was left behind"
    assert rec.get_completed_frames(cut) == at + 1 and (cut / f"state_{at:04d}.npz").exists()
    with np.load(cut / f"state_{at:04d}.npz") as st:
        p_at, _ = rec.load_frame(whole, at)
        tol = 2e-3 if zstd else 1e-6  # the lossy codec's quantum is 1e-3
        assert np.abs(st["positions"].astype(np.float32) - p_at).max() <= tol * max(1.0, float(np.abs(p_at).max()))
    ext = "zstd" if zstd else "npz"
    for k in range(at + 1):  # nothing fell back to a keyframe: the bytes of the uninterrupted run, the cut frame included
        got = (cut / f"frame_{k:04d}.{ext}").read_bytes()
        assert got == (whole / f"frame_{k:04d}.{ext}").read_bytes(), k
        if zstd:
            assert got[0] == (1 if k == 0 else 2), k
    assert (cut / f"frame_{cut_frame:04d}.{ext}").exists()
    rec.record(dict(cfg, session_name="cut"), resume=True, root=tmp_path, quiet=True)
    assert rec.get_completed_frames(cut) == total
    for k in range(total):
        a, _ = rec.load_frame(cut, k)
        b, _ = rec.load_frame(whole, k)
        assert np.abs(a - b).max() <= (4e-3 if zstd else 1e-5), k
    assert json.loads((cut / "metadata.json").read_text())["pipeline"] is True
