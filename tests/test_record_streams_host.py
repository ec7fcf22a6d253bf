"""record() itself with all three side files on (diagnostics.jsonl, groups.jsonl, pairs.jsonl), driven by a stand-in
handle without a device or libnbmi.so: which frames each file holds, the sequential against the pipelined loop, an
interrupt followed by a resume, --extend, and that every handle is closed exactly once.  Only record, extend_recording
and the files on disk are used."""
import json

import numpy as np
import pytest

N, FRAMES, SUBSTEPS = 12, 57, 2
EVERY = {"diagnostics.jsonl": 4, "groups.jsonl": 3, "pairs.jsonl": 5}


class Handle:
    """The backend object of both loops.  The state is (x, v, m); step_many is x += v * dt per step with v constant, and
    every answer is a pure function of the state, so a handle recreated from a checkpoint continues bit for bit.  The
    frame calls follow the library's rules: two slots, the snapshot and the delta chain advance at the begin."""

    def __init__(self, world, x, v, m):
        self.world, self.x, self.v, self.m = world, np.array(x, np.float64), np.array(v, np.float64), np.array(m, np.float64)
        self.steps = self.closed = self.knn_calls = 0
        self.prev, self.slots, self.seq, self.n_groups = None, {}, 0, None

    # -- stepping
    def step_many(self, dt, substeps):
        self.world.before_step()  # (an interrupt arrives here: the device stands at the frame before)
        for _ in range(substeps):
            self.x = self.x + self.v * dt
        self.steps += substeps

    def step_count(self):
        return self.steps

    def close(self):
        self.closed += 1

    # -- state, colours, frames
    def get_positions_f64(self):
        return self.x.copy()

    def get_velocities(self):
        return self.v.copy()

    def get_positions(self):
        return self.x.astype(np.float32)

    def get_colors(self):
        return (0.5 + 0.5 * np.cos(0.3 * self.x)).astype(np.float32)

    def compute_colors(self, max_speed):
        assert max_speed == 15.0

    def frame_set_previous(self, p, c):
        self.prev = (np.array(p, np.float32), np.array(c, np.float32))

    def frame_keyframe(self):
        self.prev = (self.get_positions(), self.get_colors())
        return self.prev[0].copy(), self.prev[1].copy()

    def frame_delta(self):
        from tools import record as rec
        assert self.prev is not None, "a delta frame without a previous one"
        a, b = rec.delta_quantize(self.get_positions(), self.prev[0]), rec.delta_quantize(self.get_colors(), self.prev[1])
        self.prev = (self.prev[0] + a.astype(np.float32) / 1000.0, self.prev[1] + b.astype(np.float32) / 1000.0)
        return a, b

    def frame_begin(self, kind="f32", max_speed=15.0):
        self.compute_colors(max_speed)
        free = [k for k in range(2) if k not in self.slots]
        assert free, "no free frame slot"
        a, b = {"f32": lambda: (self.get_positions(), self.get_colors()), "key": self.frame_keyframe,
                "delta": self.frame_delta}[kind]()
        self.seq += 1
        self.slots[free[0]] = (self.seq, kind, self.steps, a, b)
        return free[0]

    def frame_wait(self, slot):
        return self.slots[slot][3:]

    def frame_release(self, slot):
        del self.slots[slot]

    def frames_pending(self):
        return [(k, s[1], s[2]) for k, s in sorted(self.slots.items(), key=lambda kv: kv[1][0])]

    # -- queries
    def diagnostics(self, potential=True):
        from nbody.gpu_backend import Diagnostics
        m, x, v = self.m[:, None], self.x, self.v
        kin = float(0.5 * np.sum(m * v * v))
        pot = -float(np.sum(self.m / (1.0 + np.sqrt(np.sum(x * x, axis=1)))))
        return Diagnostics(mass=float(np.sum(m)), center_of_mass=tuple(float(c) for c in np.sum(m * x, axis=0) / np.sum(m)),
                           momentum=tuple(float(c) for c in np.sum(m * v, axis=0)),
                           angular_momentum=tuple(float(c) for c in np.sum(m * np.cross(x, v), axis=0)),
                           kinetic=kin, potential=pot, total=kin + pot, terms=len(x) * len(x))

    def force_precision_share(self):
        return float(np.mean(self.x[:, 0] > 0.0)), False

    def _d2(self):
        d = self.x[:, None, :] - self.x[None, :, :]
        return np.sum(d * d, axis=2)

    def knn(self, k, evals=False):
        assert k == 1
        self.knn_calls += 1
        d2 = self._d2()
        np.fill_diagonal(d2, np.inf)
        return d2.min(axis=1), self.m.copy()

    def find_groups(self, link, evals=False):
        near = self._d2() <= link * link
        labels = np.arange(len(self.x))
        for _ in range(len(labels)):  # smallest body index of the connected component
            labels = np.array([labels[near[i]].min() for i in range(len(labels))])
        self.n_groups = len(set(labels.tolist()))
        return labels.astype(np.int32)

    def group_catalogue(self, link, min_members=20, capacity=None):
        labels = self.find_groups(link)
        groups = [(int(np.sum(labels == g)), int(g)) for g in sorted(set(labels.tolist()))]
        groups = sorted((g for g in groups if g[0] >= min_members), key=lambda g: (-g[0], g[1]))
        rows = groups[:capacity]
        sel = [labels == g for _, g in rows]
        mass = [float(np.sum(self.m[s])) for s in sel]

        def mean(a):
            return np.array([np.sum(self.m[s, None] * a[s], axis=0) / w for s, w in zip(sel, mass)]).reshape(-1, 3)
        return {"count": len(groups), "label": np.array([g for _, g in rows], np.int32),
                "members": np.array([c for c, _ in rows], np.int64), "mass": np.array(mass), "center": mean(self.x),
                "velocity": mean(self.v), "lo": np.array([self.x[s].min(axis=0) for s in sel]).reshape(-1, 3),
                "hi": np.array([self.x[s].max(axis=0) for s in sel]).reshape(-1, 3)}

    def pair_counts(self, edges, evals=False):
        d2 = self._d2()[np.triu_indices(len(self.x), 1)]
        within = [int(np.sum(d2 <= e * e)) for e in edges]
        return np.array([b - a for a, b in zip(within[:-1], within[1:])], np.int64), within[0]


class World:
    """Stands in for nbody.gpu_backend: hands out the handles, keeps them, and interrupts the n-th step_many call."""

    def __init__(self, monkeypatch):
        import nbody.gpu_backend as gb
        self.handles, self.calls, self.interrupt_at = [], 0, None
        monkeypatch.setattr(gb, "get_backend", lambda: (gb.Backend.HIP, "stand-in"))
        monkeypatch.setattr(gb, "create_gpu_simulation", self.create)

    def create(self, positions, velocities, masses, G, softening, damping, **kw):
        self.handles.append(Handle(self, positions, velocities, masses))
        return self.handles[-1]

    def before_step(self):
        self.calls += 1
        if self.interrupt_at is not None and self.calls == self.interrupt_at + 1:
            self.interrupt_at = None
            raise KeyboardInterrupt


def _config(name, zstd, pipeline=False, frames=FRAMES):
    cfg = {"session_name": name, "num_bodies": N, "total_frames": frames, "substeps": SUBSTEPS, "dt_per_frame": 0.05,
           "G": 1.0, "softening": 0.1, "damping": 1.0, "theta": 0.5, "distribution": "galaxy", "spawn_radius": 10.0,
           "seed": 11, "diagnostics_every": EVERY["diagnostics.jsonl"],
           "groups": {"every": EVERY["groups.jsonl"], "link": "auto", "min_members": 2},
           "pairs": {"every": EVERY["pairs.jsonl"], "edges": "auto"}}
    if zstd:
        cfg["zstd"] = True
    if pipeline:
        cfg["pipeline"] = True
    return cfg


def _files(d, pattern):
    return {p.name: p.read_bytes() for p in sorted(d.glob(pattern))}


def _output(d):
    """every frame file and the three side files of a session, as bytes"""
    return {**_files(d, "frame_*"), **{name: (d / name).read_bytes() for name in EVERY}}


def _line_frames(d, name):
    return [json.loads(line)["frame"] for line in (d / name).read_text().splitlines()]


def _check_lines(d, frames):
    for name, k in EVERY.items():
        first = [-1] if name == "diagnostics.jsonl" else []
        assert _line_frames(d, name) == first + [f for f in range(frames) if (f + 1) % k == 0], name


def _check_left_behind(world, d):
    assert world.handles and [h.closed for h in world.handles] == [1] * len(world.handles), "close() not exactly once"
    assert not list(d.glob(".*.part")), "a partial file was left behind"


@pytest.fixture(params=[False, True], ids=["npz", "zstd"])
def zstd(request):
    from tools import record as rec
    if request.param:
        try:
            rec._load_zstd()
        except RuntimeError:
            pytest.skip("no libzstd")
    return request.param


@pytest.fixture
def whole(tmp_path, monkeypatch, zstd):
    """the uninterrupted sequential session: (directory, its output)"""
    from tools import record as rec
    world = World(monkeypatch)
    d = rec.record(_config("whole", zstd), root=tmp_path, quiet=True)
    _check_left_behind(world, d)
    assert len(_files(d, "frame_*")) == FRAMES
    return d, _output(d)


def test_each_file_holds_its_frames_and_metadata_the_resolved_auto(whole, monkeypatch):
    from tools import record as rec
    d, _ = whole
    _check_lines(d, FRAMES)
    first = json.loads((d / rec.DIAGNOSTICS_FILE).read_text().splitlines()[0])
    assert first["frame"] == -1 and first["abs_momentum"] > 0.0 and first["steps"] == 0
    assert all("abs_momentum" not in r for r in rec.read_diagnostics(d / rec.DIAGNOSTICS_FILE)[1:])
    meta = rec.load_metadata(d)
    link, edges = meta["groups"]["link"], meta["pairs"]["edges"]
    assert isinstance(link, float) and link > 0.0 and meta["groups"] == {"every": 3, "link": link, "min_members": 2}
    assert isinstance(edges, list) and len(edges) == 13 and meta["pairs"] == {"every": 5, "edges": edges}
    assert all(r["link"] == link for r in rec.read_diagnostics(d / rec.GROUPS_FILE))
    assert all(r["edges"] == edges for r in rec.read_diagnostics(d / rec.PAIRS_FILE))
    assert sorted(p.name for p in d.glob("state_*")) == ["state_0049.npz"]


def test_pipelined_session_writes_the_same_bytes(whole, tmp_path, monkeypatch, zstd):
    from tools import record as rec
    d, want = whole
    world = World(monkeypatch)
    p = rec.record(_config("whole", zstd, pipeline=True), root=tmp_path / "piped", quiet=True)
    _check_left_behind(world, p)
    assert _output(p) == want

    def rest(meta):
        return {k: v for k, v in meta.items() if k not in ("start_time", "start_datetime", "pipeline")}
    assert rest(rec.load_metadata(p)) == rest(rec.load_metadata(d)) and rec.load_metadata(p)["pipeline"] is True


@pytest.mark.parametrize("pipeline", [False, True], ids=["sequential", "pipelined"])
@pytest.mark.parametrize("at", [2, 50, 51])
def test_interrupt_then_resume_gives_the_uninterrupted_output(whole, tmp_path, monkeypatch, zstd, pipeline, at):
    from tools import record as rec
    _, want = whole
    world = World(monkeypatch)
    world.interrupt_at = at  # raised from the step_many call of frame `at`
    cfg = _config("cut", zstd, pipeline)
    with pytest.raises(KeyboardInterrupt):
        rec.record(cfg, root=tmp_path, quiet=True)
    d = rec.get_recording_dir("cut", tmp_path)
    _check_left_behind(world, d)
    assert rec.get_completed_frames(d) == at and (d / f"state_{at - 1:04d}.npz").exists()
    _check_lines(d, at)
    rec.record(rec.load_metadata(d), resume=True, root=tmp_path, quiet=True)
    _check_left_behind(world, d)
    assert len(world.handles) == 2 and world.handles[1].knn_calls == 0, '"auto" was taken again on the resume'
    assert _output(d) == want


def test_extend_continues_all_three_files(whole, tmp_path, monkeypatch, zstd):
    from tools import record as rec
    d, _ = whole
    world = World(monkeypatch)
    assert rec.extend_recording("whole", 6, root=tmp_path) == d
    _check_left_behind(world, d)
    assert world.handles[0].knn_calls == 0 and rec.load_metadata(d)["total_frames"] == FRAMES + 6
    assert rec.get_completed_frames(d) == FRAMES + 6
    _check_lines(d, FRAMES + 6)
    longer = rec.record(_config("longer", zstd, frames=FRAMES + 6), root=tmp_path, quiet=True)
    assert _output(d) == _output(longer)
