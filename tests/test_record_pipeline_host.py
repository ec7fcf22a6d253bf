"""Asynchronous frames, host side: the C ABI declares and exports the four calls, and the recorder's pipelined loop
(tools.record.record_pipelined) driven by a stand-in backend without a device - order of the files, slot discipline,
checkpoints, and an interrupt at every distinct point followed by a resume."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FRAME_CALLS = ("nbmi_frame_begin", "nbmi_frame_wait", "nbmi_frame_release", "nbmi_frame_pending")


def test_header_declares_and_library_exports_the_frame_calls():
    import nbmi_native
    text = open(os.path.join(ROOT, "include", "nbmi.h")).read()
    for name in FRAME_CALLS:
        assert re.search(r"^int %s\(nbmi_sim \*sim" % name, text, re.M), f"include/nbmi.h does not declare {name}"
        assert name in nbmi_native.PROTOTYPES
    assert re.search(r"^#define NBMI_FRAME_SLOTS 2$", text, re.M)
    for k, name in enumerate(("NBMI_FRAME_F32", "NBMI_FRAME_KEY", "NBMI_FRAME_DELTA_I16")):
        assert re.search(r"^#define %s %d\b" % (name, k), text, re.M)
    lib = ctypes.CDLL(nbmi_native.LIB_PATH)
    for name in FRAME_CALLS:
        assert hasattr(lib, name), f"libnbmi.so lacks {name}"


def test_cli_flag_metadata_key_and_status(tmp_path, capsys):
    from tools import record as rec
    ap = rec.build_parser()
    cfg = rec.build_config(ap.parse_args(["--preset", "quick_galaxy", "--pipeline"]))
    assert cfg["pipeline"] is True
    assert "pipeline" not in rec.build_config(ap.parse_args(["--preset", "quick_galaxy"]))  # the default writes no key
    for name, c in (("on", cfg), ("off", {k: v for k, v in cfg.items() if k != "pipeline"})):
        rec.save_metadata(rec.get_recording_dir(name, tmp_path), c, 0.0)
        capsys.readouterr()
        assert rec.show_status(name, root=tmp_path)
        assert f"Pipeline: {name}" in capsys.readouterr().out
    assert rec.load_metadata(rec.get_recording_dir("on", tmp_path))["pipeline"] is True


# ---- a stand-in for the backend object: the "state" is the number of steps taken since the start of the recording ------
N = 11


def _frame_of(total_steps):
    i = np.arange(N * 3, dtype=np.float64).reshape(N, 3)
    p = (80.0 * np.sin(0.37 * i + 0.05 * total_steps) + 0.4 * total_steps).astype(np.float32)
    c = (0.5 + 0.5 * np.cos(0.11 * i + 0.03 * total_steps)).astype(np.float32)
    return p, c


class FakeSim:
    """step_many / frame_begin / frame_wait / frame_release / frames_pending / step_count with the library's rules: two
    slots, a snapshot is taken at the begin, the delta chain advances at the begin, pending frames in begin order."""
    SLOTS = 2

    def __init__(self, rec, base_steps=0, log=None):
        self.rec = rec
        self.base = base_steps   # steps the restored state had already taken
        self.steps = 0           # step_count(): since this handle was created
        self.slots = {}          # slot -> (seq, kind, steps, a, b)
        self.seq = 0
        self.prev = None
        self.log = log if log is not None else []
        self.max_held = 0
        self.hooks = {}

    def _hook(self, name):
        h = self.hooks.get(name)
        if h:
            h()

    def step_many(self, dt, substeps):
        self.steps += substeps
        self.log.append(("step", self.steps))
        self._hook("after_step")

    def step_count(self):
        return self.steps

    def frame_set_previous(self, p, c):
        self.prev = (np.array(p, dtype=np.float32), np.array(c, dtype=np.float32))

    def frame_begin(self, kind="f32", max_speed=15.0):
        assert max_speed == 15.0
        free = [k for k in range(self.SLOTS) if k not in self.slots]
        if not free:
            raise ValueError("no free frame slot")
        p, c = _frame_of(self.base + self.steps)
        if kind == "delta":
            if self.prev is None:
                raise ValueError("no previous frame")
            a, b = self.rec.delta_quantize(p, self.prev[0]), self.rec.delta_quantize(c, self.prev[1])
            self.prev = (self.prev[0] + a.astype(np.float32) / 1000.0, self.prev[1] + b.astype(np.float32) / 1000.0)
        else:
            a, b = p, c
            if kind == "key":
                self.prev = (p.copy(), c.copy())
        self.seq += 1
        self.slots[free[0]] = (self.seq, kind, self.steps, a, b)
        self.max_held = max(self.max_held, len(self.slots))
        self.log.append(("begin", free[0], self.steps))
        self._hook("after_begin")
        return free[0]

    def frame_wait(self, slot):
        _, _, _, a, b = self.slots[slot]
        self._hook("in_wait")
        a, b = a.view(), b.view()
        a.flags.writeable = b.flags.writeable = False
        return a, b

    def frame_release(self, slot):
        del self.slots[slot]
        self.log.append(("release", slot))

    def frames_pending(self):
        return [(k, v[1], v[2]) for k, v in sorted(self.slots.items(), key=lambda kv: kv[1][0])]


def _session(rec, rec_dir, total, substeps, zstd, every=0, hooks=None, log=None):
    """What record() does around the loop, with the stand-in: resume from the latest checkpoint, then the pipelined loop."""
    start, base = 0, 0
    completed = rec.get_completed_frames(rec_dir)
    if completed:
        f, k = rec.find_latest_state(rec_dir, completed)
        if f is not None:
            with np.load(f) as st:
                base = int(st["steps"])
            start = k + 1
    sim = FakeSim(rec, base, log)
    sim.hooks = hooks or {}
    if zstd and start > 0:
        sim.frame_set_previous(*rec.load_frame(rec_dir, start - 1))
    events = sim.log

    def write_diag(frame):
        if every > 0 and (frame + 1) % every == 0:
            assert any(p.exists() for p in rec._frame_paths(rec_dir, frame)), "diagnostics before its frame"
            events.append(("diag", frame))

    def write_state(frame, compressed=False):
        assert any(p.exists() for p in rec._frame_paths(rec_dir, frame)), "checkpoint before its frame file"
        assert start - 1 + sim.step_count() // substeps == frame, "checkpoint of a state that is not this frame's"
        assert not sim.frames_pending(), "checkpoint while a frame is in flight"
        steps = np.int64(sim.base + sim.steps)
        rec._atomically(rec_dir / f"state_{frame:04d}.npz", lambda f: np.savez(f, steps=steps))
        events.append(("state", frame))

    try:
        rec.record_pipelined(sim, rec_dir, start, total, substeps, 0.01, zstd, every, write_diag, write_state)
    finally:
        assert not sim.slots, "a slot was not released"
        assert sim.max_held <= 2
    return sim


def _frame_files(d):
    return {p.name: p.read_bytes() for p in sorted(d.glob("frame_*"))}


def _need_zstd(rec, zstd):
    if zstd:
        try:
            rec._load_zstd()
        except RuntimeError:
            pytest.skip("no libzstd")


@pytest.mark.parametrize("zstd", [False, True])
def test_pipelined_loop_order_slots_and_checkpoints(tmp_path, monkeypatch, zstd):
    from tools import record as rec
    _need_zstd(rec, zstd)
    d = rec.get_recording_dir("whole", tmp_path)
    written = []
    real = rec._atomically

    def noting(path, write):
        real(path, write)
        written.append(path.name)

    monkeypatch.setattr(rec, "_atomically", noting)
    total, substeps = 104, 3
    sim = _session(rec, d, total, substeps, zstd, every=7)
    ext = "zstd" if zstd else "npz"
    assert [w for w in written if w.startswith("frame_")] == [f"frame_{k:04d}.{ext}" for k in range(total)]
    assert rec.get_completed_frames(d) == total
    assert [e[1] for e in sim.log if e[0] == "state"] == [49, 99]
    assert sorted(p.name for p in d.glob("state_*")) == ["state_0099.npz"]  # the older checkpoint is removed
    assert [e[1] for e in sim.log if e[0] == "diag"] == [k for k in range(total) if (k + 1) % 7 == 0]
    # overlap: frame k is begun before frame k - 1 is released, except right after a frame that was finished at once
    log = sim.log
    begins = [i for i, e in enumerate(log) if e[0] == "begin"]
    overlapped = sum(1 for i in begins[1:] if log[i + 1][0] == "release")
    assert overlapped >= total - 2 - total // 7 - 2
    # the content: what the sequential codec gives for the same frames
    prev = None
    for k in range(total):
        p, c = _frame_of((k + 1) * substeps)
        if zstd:
            blob = rec.compress_frame(p, c, *(prev or (None, None)))
            assert (d / f"frame_{k:04d}.zstd").read_bytes() == blob, k
            prev = rec.decompress_frame(blob, *(prev or (None, None)))
        else:
            buf = io.BytesIO()
            np.savez(buf, positions=p, colors=c)
            assert (d / f"frame_{k:04d}.npz").read_bytes() == buf.getvalue(), k


POINTS = ("after_step", "after_begin", "in_wait", "in_atomically")


@pytest.mark.parametrize("zstd", [False, True])
@pytest.mark.parametrize("point", POINTS)
@pytest.mark.parametrize("nth", [1, 2, 6, 50, 51, 52])
def test_interrupt_then_resume_gives_the_uninterrupted_files(tmp_path, monkeypatch, zstd, point, nth):
    from tools import record as rec
    _need_zstd(rec, zstd)
    total, substeps = 57, 2
    whole = rec.get_recording_dir("whole", tmp_path)
    _session(rec, whole, total, substeps, zstd, every=4)
    want = _frame_files(whole)
    assert len(want) == total

    cut = rec.get_recording_dir("cut", tmp_path)
    calls = {"n": 0}

    def hook():
        calls["n"] += 1
        if calls["n"] == nth:
            raise KeyboardInterrupt

    real = rec._atomically
    if point == "in_atomically":
        def cut_short(path, write):
            if path.name.startswith("frame_"):
                calls["n"] += 1
                if calls["n"] == nth:
                    def half(f):
                        buf = io.BytesIO()
                        write(buf)
                        f.write(buf.getvalue()[: len(buf.getvalue()) // 2])
                        f.flush()
                        raise KeyboardInterrupt
                    return real(path, half)
            return real(path, write)
        monkeypatch.setattr(rec, "_atomically", cut_short)
        hooks = {}
    else:
        hooks = {point: hook}
    log = []
    with pytest.raises(KeyboardInterrupt):
        _session(rec, cut, total, substeps, zstd, every=4, hooks=hooks, log=log)
    monkeypatch.setattr(rec, "_atomically", real)
    assert not list(cut.glob(".*.part")), "a partial file was left behind"
    done = rec.get_completed_frames(cut)
    at = max(e[1] for e in log if e[0] == "step") // substeps - 1  # the frame the device stood at
    assert done == at + 1 and (cut / f"state_{at:04d}.npz").exists()
    with np.load(cut / f"state_{at:04d}.npz") as st:
        assert int(st["steps"]) == (at + 1) * substeps  # the checkpoint is the state of the last frame on disk
    got = _frame_files(cut)
    assert got == {k: v for k, v in want.items() if k in got}, "frames written around the interrupt differ"
    if zstd and at > 0:
        assert (cut / f"frame_{at:04d}.zstd").read_bytes()[0] == 2  # a delta frame, not a keyframe fall-back
    _session(rec, cut, total, substeps, zstd, every=4)
    assert _frame_files(cut) == want
