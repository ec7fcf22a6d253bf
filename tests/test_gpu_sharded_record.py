"""GPU tests of the multi-GPU shard engine (as virtual shards on one GPU) and of record()."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("knobs", [{}, {"NBMI_SPLIT_WAVES": "0"}, {"NBMI_SPLIT_WAVES": "0", "NBMI_WALK_PAIR": "2"}],
                         ids=["split-walk", "one-wave-walk", "one-wave-walk-home-cut"])
def test_virtual_shards_bit_identical_to_single_handle(gpu, monkeypatch, knobs):
    """Three handles on one GPU play three ranks: each integrates its key-range, rows are exchanged
    through device buffers exactly as nbody/sharded.py does (the all-gather itself replaced by
    torch.cat).  The result must equal the unsharded handle bit for bit - with every walk form: the split walk
    this size gets by default, the one-wave walk, and the one-wave walk that cuts the node array at the wave's
    own leaves (the default from 1.5 M bodies on; shard ranges start at multiples of 64 ranks for its sake)."""
    import torch
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    from nbody.gpu_backend import HIPBarnesHutSimulation
    from nbody.sharded import HipShardEngine, ShardedBarnesHut, shard_bounds
    g = golden("tree_collision_2048")
    n = 2001  # ragged
    pos, vel, mass = g["pos"][:n], g["vel"][:n], g["mass"][:n]
    G, eps = float(g["G"]), float(g["eps"])
    world = 3
    single = HIPBarnesHutSimulation(pos, vel, mass, G, eps, 1.0, 0.5)
    engines = [HipShardEngine(pos, vel, mass, G, eps, 1.0, 0.5, 0) for _ in range(world)]
    shards = [ShardedBarnesHut(e, n, r, world, dist=None) for r, e in enumerate(engines)]
    per = shards[0].per
    assert [(s.begin, s.end) for s in shards] == [shard_bounds(n, world, r)[1:] for r in range(world)]
    for _ in range(5):
        single.step(0.05)
        for s in shards:
            s.engine.step(0.05)
            s.engine.export_rows(s.mine)
        full = torch.cat([s.mine for s in shards], dim=0)
        assert full.shape == (per * world, 8)
        for s in shards:
            s.engine.import_rows(full, n)
    ref_p, ref_v = single.get_positions_f64(), single.get_velocities()
    for e in engines:
        assert np.array_equal(e.sim.get_positions_f64(), ref_p)
        assert np.array_equal(e.sim.get_velocities(), ref_v)
    # a sharded handle refuses multi-substep calls (the other ranks' rows would be missing)
    with pytest.raises(RuntimeError, match="sharded handle"):
        engines[0].sim.step_many(0.05, 2)
    # world_size 1 goes through the same class without any exchange
    one = ShardedBarnesHut(HipShardEngine(pos, vel, mass, G, eps, 1.0, 0.5, 0), n, 0, 1)
    one.step(0.05, 5)
    assert np.array_equal(one.engine.sim.get_positions_f64(), ref_p)


def test_direct_virtual_shards_bit_identical(gpu):
    """All-pairs kernel sharded by body index through the same row exchange: three handles on one GPU."""
    import torch
    from nbody.gpu_backend import HIPDirectSimulation
    from nbody.sharded import HipShardEngine, ShardedBarnesHut
    g = golden("direct_cluster_2048")
    n = 1999
    pos, vel, mass = g["pos"][:n], g["vel"][:n], g["mass"][:n]
    G, eps = float(g["G"]), float(g["eps"])
    world = 3
    single = HIPDirectSimulation(pos, vel, mass, G, eps, 1.0)
    engines = [HipShardEngine(pos, vel, mass, G, eps, 1.0, 0.0, 0, method="direct") for _ in range(world)]
    shards = [ShardedBarnesHut(e, n, r, world, dist=None) for r, e in enumerate(engines)]
    for _ in range(4):
        single.step(0.02)
        for s in shards:
            s.engine.step(0.02)
            s.engine.export_rows(s.mine)
        full = torch.cat([s.mine for s in shards], dim=0)
        for s in shards:
            s.engine.import_rows(full, n)
    for e in engines:
        assert np.array_equal(e.sim.get_positions_f64(), single.get_positions_f64())
        assert np.array_equal(e.sim.get_velocities(), single.get_velocities())


def test_rccl_one_rank_group_stream_ordered_exchange(gpu):
    """The production exchange path with the real RCCL backend, as far as one GPU allows: a process
    group of one rank, rows packed / all-gathered / unpacked on the library's own stream (no host
    synchronisation inside a step).  Must equal the plain handle bit for bit."""
    import socket
    import torch
    import torch.distributed as dist
    from nbody.gpu_backend import HIPBarnesHutSimulation
    from nbody.sharded import HipShardEngine, ShardedBarnesHut
    g = golden("tree_galaxy_2048")
    pos, vel, mass = g["pos"], g["vel"], g["mass"]
    G, eps = float(g["G"]), float(g["eps"])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    torch.cuda.set_device(0)
    try:
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
    except Exception as ex:  # noqa: BLE001 - an environment without a usable RCCL is not a product failure
        pytest.skip(f"RCCL process group unavailable here: {ex}")
    import os
    try:
        single = HIPBarnesHutSimulation(pos, vel, mass, G, eps, 1.0, 0.5)
        single.step_many(0.05, 7)
        for opt_in in (False, True):  # default: host-synchronised exchange; NBMI_EXCHANGE_SYNC=0: stream-ordered
            if opt_in:
                os.environ["NBMI_EXCHANGE_SYNC"] = "0"
            try:
                sh = ShardedBarnesHut(HipShardEngine(pos, vel, mass, G, eps, 1.0, 0.5, 0), len(pos), 0, 1, dist)
            finally:
                os.environ.pop("NBMI_EXCHANGE_SYNC", None)
            assert (sh.shared is not None) == opt_in
            sh.step(0.05, 7)
            sh.engine.sim.sync()
            assert np.array_equal(sh.engine.sim.get_positions_f64(), single.get_positions_f64())
            assert np.array_equal(sh.engine.sim.get_velocities(), single.get_velocities())
    finally:
        dist.destroy_process_group()


class _ThreadComm:
    """The collectives of nbody.sharded.LetBarnesHut between `world` Python threads that play the ranks."""

    def __init__(self, world):
        import threading
        self.world, self.bar, self.slots = world, threading.Barrier(world), [None] * world

    def bind(self, rank):
        comm = self

        class Bound:
            def _swap(self, mine):
                # a real collective reads `mine` in the order of the stream it is enqueued on (the library's, since
                # round 3); these threads read each other's buffers directly, so the producer's stream is drained first
                import torch
                torch.cuda.current_stream().synchronize()
                comm.slots[rank] = mine
                comm.bar.wait()
                got = list(comm.slots)
                comm.bar.wait()
                return got

            def all_reduce_max(self, t):
                import torch
                m = torch.stack(self._swap(t.clone())).max(dim=0).values
                t.copy_(m)
                torch.cuda.synchronize()
                comm.bar.wait()

            def all_gather(self, full, mine):
                import torch
                full.copy_(torch.cat(self._swap(mine), dim=0))
                torch.cuda.synchronize()
                comm.bar.wait()

            def all_to_all_counts(self, send_counts):
                return np.array([c[rank] for c in self._swap(np.array(send_counts))], dtype=np.int64)

            def counts_matrix(self, send_row):
                """every rank's row on every rank (DistComm.counts_matrix): the collective capacity checks and the
                system-wide force-precision vote need it"""
                return np.stack(self._swap(np.array(send_row, dtype=np.int64)))

            def all_to_all_rows(self, recv, send, recv_counts, send_counts):
                import torch
                got = self._swap((send, np.array(send_counts)))
                off = 0
                for j in range(comm.world):
                    sj, cj = got[j]
                    start, c = int(cj[:rank].sum()), int(cj[rank])
                    assert c == int(recv_counts[j])
                    recv[off:off + c].copy_(sj[start:start + c])
                    off += c
                torch.cuda.synchronize()
                comm.bar.wait()

        return Bound()


def _run_ranks(steppers, comm, dt, steps):
    import threading
    world = len(steppers)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            steppers[r].step(dt, steps)
            out[r] = steppers[r].gather_state()
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            comm.bar.abort()

    ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join(300) for t in ts]
    assert not errs, errs
    return out


def test_owner_mode_three_ranks_agree_with_single_handle(gpu):
    """Multi-GPU stage 2 (north_star form): owned key ranges, body migration, every rank's octree cut into its piece of
    the ONE global pre-order array, pruned pieces exchanged.  Three threads on one GPU play three ranks through
    LetBarnesHut.step itself.  Same accepted sets as the single handle; in the default force precision the fp32 waves'
    partial sums associate differently (which 64 bodies form a wave differs), so the comparison is a tolerance:
    <= 1e-7 of the largest coordinate after 5 steps."""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    from nbody.sharded import HipLetEngine, LetBarnesHut
    from tools.presets import generate_distribution
    np.random.seed(7)
    n = 60_001
    pos, vel, mass = generate_distribution("galaxy", n, 500.0, 0.15)
    mass = mass * np.random.uniform(0.5, 1.5, n)
    G, eps, theta = 0.15, 3.0, 0.5
    world, steps, dt = 3, 5, 0.05
    single = HIPBarnesHutSimulation(pos, vel, mass, G, eps, 1.0, theta)
    single.step_many(dt, steps)
    ref_p, ref_v = single.get_positions_f64(), single.get_velocities()
    own_nodes = single.tree_stats()["num_nodes"]

    comm = _ThreadComm(world)
    engines = [HipLetEngine(pos, vel, mass, G, eps, 1.0, theta, 0, r, world) for r in range(world)]
    steppers = [LetBarnesHut(e, r, world, comm.bind(r)) for r, e in enumerate(engines)]
    out = _run_ranks(steppers, comm, dt, steps)
    scale = np.abs(ref_p).max()
    for r in range(world):
        err = np.abs(out[r][0] - ref_p).max() / scale
        verr = np.abs(out[r][1] - ref_v).max() / np.abs(ref_v).max()
        print(f"rank {r}: owns {engines[r].sim.n} bodies, received tree rows per source {engines[r].let_counts.tolist()} "
              f"(single-GPU tree {own_nodes}), sent {engines[r].wire_bytes} B, migrated {engines[r].migrated}; "
              f"pos err {err:.2e} vel err {verr:.2e}")
        assert err <= 1e-7 and verr <= 1e-5
        assert np.array_equal(out[r][0], out[0][0])  # every rank gathered the same state
    counts = [e.sim.n for e in engines]
    assert sum(counts) == n and max(counts) <= 1.1 * n / world + 64  # re-balanced by the sampled splitters
    # a rank receives pruned trees; at 20 k bodies per rank much of a neighbour's tree is still "near" - the
    # pruning pays at bench sizes (scripts/gpu_let_probe.py)
    for e in engines:
        assert e.let_counts[e.rank] == 0 and 0 < e.let_counts[(e.rank + 1) % world] <= 1.6 * max(counts)
    # an owner handle refuses the single-GPU entry points
    with pytest.raises(RuntimeError, match="owner mode"):
        engines[0].sim.step(dt)
    for e in engines:
        e.sim.close()


@pytest.mark.parametrize("dist,n,world,theta,eps", [
    ("galaxy", 60_001, 3, 0.5, 3.0),      # deep cells below theta * eps: opened by nobody, pruned for everybody
    ("galaxy", 50_000, 8, 0.5, 0.05),     # every boundary deep inside the core
    ("collision", 30_000, 5, 0.9, 0.5),   # theta > 1/sqrt(3): a body may accept a cell it sits in
    ("cluster", 20_000, 2, 0.3, 0.2),
    ("galaxy", 700, 8, 0.5, 1.0),         # ~90 bodies per rank
    ("galaxy", 37, 8, 0.7, 1.0),          # a handful of bodies per rank, some ranks may own none
    ("galaxy", 9, 8, 0.5, 1.0),
    ("galaxy", 5, 8, 0.5, 1.0),           # fewer bodies than ranks
    ("galaxy", 20_000, 4, 0.0, 1.0),      # theta = 0: every cell is opened (direct sum through the tree)
    ("galaxy", 20_000, 4, 0.5, 0.0),      # softening 0: the guarded walk (pairs at dist_sq <= eps^2 skipped)
])
def test_owner_mode_walks_the_single_gpu_octree(gpu, dist, n, world, theta, eps):
    """The ranks' pieces put together are the single handle's pre-order array (global moments on the cells that span
    ranks, cells born on a boundary inserted, copies dropped): with float64 forces every body adds the same
    contributions in the same order as on one GPU.  Only the split walk of small systems associates its per-part sums
    by array position: 1e-13 of the largest coordinate after 4 steps, not bit for bit."""
    _owner_against_single(dist, n, world, theta, eps, 1.0)


def test_owner_mode_damped_walks_the_single_gpu_octree(gpu):
    """The same with damping 0.99 in the fused kick-drift of every rank's walk."""
    _owner_against_single("galaxy", 60_001, 3, 0.5, 3.0, 0.99)


def _owner_against_single(dist, n, world, theta, eps, damping):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    from nbody.sharded import HipLetEngine, LetBarnesHut
    from tools.presets import generate_distribution
    np.random.seed(11)
    pos, vel, mass = generate_distribution(dist, n, 300.0, 0.2)
    mass = mass * np.random.uniform(0.5, 1.5, n)
    G, dt, steps = 0.2, 0.02, 4
    single = HIPBarnesHutSimulation(pos, vel, mass, G, eps, damping, theta)
    single.set_force_precision("f64")
    single.step_many(dt, steps)
    ref_p, ref_v = single.get_positions_f64(), single.get_velocities()
    single.close()
    comm = _ThreadComm(world)
    engines = [HipLetEngine(pos, vel, mass, G, eps, damping, theta, 0, r, world) for r in range(world)]
    for e in engines:
        e.sim.set_force_precision("f64")
    steppers = [LetBarnesHut(e, r, world, comm.bind(r)) for r, e in enumerate(engines)]
    out = _run_ranks(steppers, comm, dt, steps)
    err = np.abs(out[0][0] - ref_p).max() / np.abs(ref_p).max()
    verr = np.abs(out[0][1] - ref_v).max() / np.abs(ref_v).max()
    print(f"{dist} {n} bodies on {world} ranks, theta {theta}: owned {[e.sim.n for e in engines]}, pos {err:.1e} vel {verr:.1e}")
    assert err <= 1e-13 and verr <= 1e-11
    assert sum(e.sim.n for e in engines) == n
    for e in engines:
        e.sim.close()


def test_owner_mode_one_rank_is_the_single_handle(gpu):
    """World size 1 goes through the same calls with no collective and must equal the plain handle bit for bit."""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    from nbody.sharded import HipLetEngine, LetBarnesHut
    g = golden("tree_collision_2048")
    n = 2001
    pos, vel, mass = g["pos"][:n], g["vel"][:n], g["mass"][:n] * np.linspace(0.5, 2.0, n)
    G, eps = float(g["G"]), float(g["eps"])
    single = HIPBarnesHutSimulation(pos, vel, mass, G, eps, 1.0, 0.5)
    single.step_many(0.05, 6)
    one = LetBarnesHut(HipLetEngine(pos, vel, mass, G, eps, 1.0, 0.5, 0, 0, 1), 0, 1)
    one.step(0.05, 6)
    p1, v1 = one.gather_state()
    assert np.array_equal(p1, single.get_positions_f64()) and np.array_equal(v1, single.get_velocities())


def test_record_writes_reference_format_and_resumes(gpu, tmp_path, oracle):
    from tools import record as rec
    from tools.presets import generate_distribution, get_preset_config
    cfg = get_preset_config("quick_galaxy")
    cfg.update(num_bodies=3000, theta=0.5, total_frames=60, substeps=2, session_name="t_rec")
    d = rec.record(cfg, root=tmp_path, quiet=True, seed=42)
    assert rec.get_completed_frames(d) == 60
    meta = rec.load_metadata(d)
    assert meta["num_bodies"] == 3000 and meta["substeps"] == 2 and "start_datetime" in meta
    p, c = rec.load_frame(d, 59)
    assert p.dtype == np.float32 and p.shape == (3000, 3) and c.dtype == np.float32 and c.shape == (3000, 3)
    with np.load(d / "frame_0000.npz") as f:
        assert sorted(f.files) == ["colors", "positions"]
    # state checkpoint every 50 frames, keys of the reference + masses
    assert (d / "state_0049.npz").exists() and not (d / "state_0099.npz").exists()
    with np.load(d / "state_0049.npz") as st:
        assert {"positions", "velocities"} <= set(st.files)
        assert st["positions"].shape == (3000, 3) and st["velocities"].dtype == np.float64
    # the frames follow the reference's CPU loop (dt = dt_per_frame / substeps)
    np.random.seed(42)
    ip, iv, im = generate_distribution("galaxy", 3000, 500.0, 0.15)
    ref = oracle.BHStepper(ip, iv, im, 0.5, 0.15, 3.0, 1.0)
    for _ in range(60 * 2):
        ref.step(0.1)
    err = np.abs(p - ref.pos).max() / np.abs(ref.pos).max()
    print("record frame 59 rel err vs oracle", err)
    assert err < 1e-4
    assert np.abs(c - oracle.compute_colors_by_velocity(ref.vel, 15.0)).max() < 5e-3
    # resume: drop the tail, continue from state_0049 -> same frames again
    for k in range(50, 60):
        (d / f"frame_{k:04d}.npz").unlink()
    cfg2 = dict(cfg)
    d2 = rec.record(cfg2, resume=True, root=tmp_path, quiet=True)
    assert d2 == d and rec.get_completed_frames(d) == 60
    p2, _ = rec.load_frame(d, 59)
    assert np.array_equal(p2, p)
    # raw -> .zstd conversion keeps the chain loadable
    try:
        rec._load_zstd()
    except RuntimeError:
        return
    assert rec.compress_recording(d) == 60
    q, _ = rec.load_frame(d, 59)
    assert np.abs(q - p).max() < 0.06  # int16 millis quantisation accumulates over the chain


def test_device_frame_codec_is_the_host_codec_bit_for_bit(gpu):
    """int16((cur - prev) * 1000) quantised on the device against the previous DECODED frame
    (reference tools/record.py:254-262, decoder :313-322) equals tools.record.delta_quantize on the same arrays,
    the wrap-around beyond +-32.767 included; only 12 B per body cross PCIe."""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    from tools import record as rec
    g = golden("tree_galaxy_2048")
    sim = HIPBarnesHutSimulation(g["pos"], g["vel"], g["mass"], float(g["G"]), float(g["eps"]), 1.0, 0.5)
    sim.compute_colors(15.0)
    with pytest.raises(RuntimeError, match="no previous frame"):
        sim.frame_delta()
    prev_p, prev_c = sim.frame_keyframe()
    assert np.array_equal(prev_p, sim.get_positions()) and np.array_equal(prev_c, sim.get_colors())
    for k in range(6):
        if k == 3:  # a jump of > 32.767 for some bodies: the int16 cast wraps, on the device as on the host
            x, v = sim.get_positions_f64(), sim.get_velocities()
            x[::7] += [40.0, -70.0, 33.0]
            sim.set_state(x, v)
        sim.step_many(0.1, 2)
        sim.compute_colors(15.0)
        dp, dc = sim.frame_delta()
        cur_p, cur_c = sim.get_positions(), sim.get_colors()
        assert np.array_equal(dp, rec.delta_quantize(cur_p, prev_p)), k
        assert np.array_equal(dc, rec.delta_quantize(cur_c, prev_c)), k
        if k == 3:
            assert (np.abs((cur_p - prev_p) * 1000) > 32767).any()
        # the decoder's reconstruction is the next frame's reference, on both sides
        prev_p = prev_p + dp.astype(np.float32) / 1000.0
        prev_c = prev_c + dc.astype(np.float32) / 1000.0
    sim.close()


def test_record_direct_zstd_extend_and_interrupt(gpu, tmp_path, monkeypatch):
    """record() with "zstd": True writes .zstd frames whose delta payload comes from the device; the files are
    byte-identical to compressing the raw frames on the host.  extend_recording = the reference's --extend
    (:1156-1199); Ctrl-C leaves a state checkpoint to resume from (:916-935)."""
    from tools import record as rec
    from tools.presets import get_preset_config
    try:
        rec._load_zstd()
    except RuntimeError:
        pytest.skip("no libzstd")
    cfg = get_preset_config("quick_galaxy")
    cfg.update(num_bodies=2000, theta=0.5, total_frames=12, substeps=2)
    raw = rec.record(dict(cfg, session_name="t_raw"), root=tmp_path, quiet=True, seed=5)
    z = rec.record(dict(cfg, session_name="t_z", zstd=True), root=tmp_path, quiet=True, seed=5)
    assert rec.get_completed_frames(z) == 12 and (z / "frame_0011.zstd").exists() and not list(z.glob("*.npz"))
    assert rec.compress_recording(raw) == 12
    for k in range(12):
        assert (z / f"frame_{k:04d}.zstd").read_bytes() == (raw / f"frame_{k:04d}.zstd").read_bytes(), k
    p11, _ = rec.load_frame(z, 11)
    # --extend: 12 -> 60 frames; no state file yet, so the run restarts from frame 0 like the reference does
    d = rec.extend_recording("t_z", 48, root=tmp_path)
    assert d == z and rec.load_metadata(z)["total_frames"] == 60 and rec.get_completed_frames(z) == 60
    assert np.array_equal(rec.load_frame(z, 11)[0], p11) and (z / "state_0049.npz").exists()
    # resume in direct-zstd mode continues the delta chain from the decoded last frame on disk
    before = [(z / f"frame_{k:04d}.zstd").read_bytes() for k in range(50, 60)]
    for k in range(50, 60):
        (z / f"frame_{k:04d}.zstd").unlink()
    rec.record(dict(rec.load_metadata(z), session_name="t_z"), resume=True, root=tmp_path, quiet=True)
    assert [(z / f"frame_{k:04d}.zstd").read_bytes() for k in range(50, 60)] == before
    # Ctrl-C in the middle of a run: the frame in flight is finished, a state file is left, resume completes
    calls = {"n": 0}
    real = rec.save_frame

    def flaky(*a, **k):
        calls["n"] += 1
        real(*a, **k)
        if calls["n"] == 7:
            raise KeyboardInterrupt

    monkeypatch.setattr(rec, "save_frame", flaky)
    with pytest.raises(KeyboardInterrupt):
        rec.record(dict(cfg, session_name="t_int"), root=tmp_path, quiet=True, seed=5)
    monkeypatch.setattr(rec, "save_frame", real)
    ti = tmp_path / "recordings" / "t_int"
    assert rec.get_completed_frames(ti) == 7 and (ti / "state_0006.npz").exists()
    rec.record(dict(cfg, session_name="t_int"), resume=True, root=tmp_path, quiet=True)
    assert rec.get_completed_frames(ti) == 12
    a, _ = rec.load_frame(ti, 11)
    b, _ = rec.load_frame(raw, 11)
    assert np.abs(a - b).max() < 0.06  # raw frames vs the (lossy) compressed copy of the uninterrupted run


@pytest.mark.parametrize("zstd", [False, True])
def test_interrupt_delivered_when_the_step_call_returns(gpu, tmp_path, monkeypatch, zstd):
    """Ctrl-C is delivered when nbmi_step returns - the device has advanced, the loop has noted nothing.
    The checkpoint must be the state of the last frame on disk: the resumed recording equals the uninterrupted one."""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    from tools import record as rec
    from tools.presets import get_preset_config
    if zstd:
        try:
            rec._load_zstd()
        except RuntimeError:
            pytest.skip("no libzstd")
    cfg = get_preset_config("quick_galaxy")
    cfg.update(num_bodies=2000, theta=0.5, total_frames=9, substeps=3, zstd=zstd)
    whole = rec.record(dict(cfg, session_name="t_whole"), root=tmp_path, quiet=True, seed=11)
    real = HIPBarnesHutSimulation.step_many
    calls = {"n": 0}

    def stepping(self, dt, substeps):
        real(self, dt, substeps)
        calls["n"] += 1
        if calls["n"] == 5:  # frame 4 has been stepped on the device, nothing of it is on disk
            raise KeyboardInterrupt

    monkeypatch.setattr(HIPBarnesHutSimulation, "step_many", stepping)
    with pytest.raises(KeyboardInterrupt):
        rec.record(dict(cfg, session_name="t_cut"), root=tmp_path, quiet=True, seed=11)
    monkeypatch.setattr(HIPBarnesHutSimulation, "step_many", real)
    cut = tmp_path / "recordings" / "t_cut"
    assert rec.get_completed_frames(cut) == 5 and (cut / "state_0004.npz").exists()
    with np.load(cut / "state_0004.npz") as st:
        p4, _ = rec.load_frame(whole, 4)
        tol = 2e-3 if zstd else 1e-6  # the lossy codec's quantum is 1e-3
        assert np.abs(st["positions"].astype(np.float32) - p4).max() <= tol * max(1.0, float(np.abs(p4).max()))
    rec.record(dict(cfg, session_name="t_cut"), resume=True, root=tmp_path, quiet=True)
    assert rec.get_completed_frames(cut) == 9
    for k in range(9):
        a, _ = rec.load_frame(cut, k)
        b, _ = rec.load_frame(whole, k)
        assert np.abs(a - b).max() <= (4e-3 if zstd else 1e-5), k


def test_owner_mode_1m_bodies_eight_ranks_100_steps_meet_the_north_star_bound(gpu, oracle):
    """Owner mode at bench scale: BASELINE config 2's 1 M bodies over EIGHT ranks (threads on one GPU through
    LetBarnesHut.step itself, collectives on the library's stream), the full 100 steps against the float64 oracle, in the
    default force precision: the same <= 1e-4 / p99.9 <= 1e-5 as the single handle's test.  (Round 2's partial cells:
    1.7e-3 after the 100 steps in every force precision - profiles/r03_owner_100_steps_partial_cells.jsonl.)"""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    from nbody.sharded import HipLetEngine, LetBarnesHut
    from test_gpu_nbody import _oracle_galaxy_1m
    n, world, dt = 1_000_000, 8, 0.05
    G, eps, theta = 0.07, 1.5, 0.5
    pos, vel, mass, ref = _oracle_galaxy_1m(oracle, 100, (10, 50, 100))
    single = HIPBarnesHutSimulation(pos, vel, mass, G, eps, 1.0, theta)
    single.step_many(dt, 100)
    single_err = float((np.abs(single.get_positions_f64() - ref[100]).max(axis=1) / np.abs(ref[100]).max()).max())
    single_all64 = single.force_precision_share()[1]
    single.close()
    comm = _ThreadComm(world)
    engines = [HipLetEngine(pos, vel, mass, G, eps, 1.0, theta, 0, r, world) for r in range(world)]
    assert all(e.stream is not None for e in engines)  # stream-ordered exchange is the default
    steppers = [LetBarnesHut(e, r, world, comm.bind(r)) for r, e in enumerate(engines)]
    done = 0
    for k in (10, 50, 100):
        out = _run_ranks(steppers, comm, dt, k - done)
        done = k
        d = np.abs(out[0][0] - ref[k]).max(axis=1) / np.abs(ref[k]).max()
        print(f"  owner mode, 1 M x 8 ranks x {k} steps: max {d.max():.3e} p99.9 {np.quantile(d, 0.999):.3e}; "
              f"received tree rows {[int(e.let_counts.sum()) for e in engines]}")
    assert d.max() <= 1e-4 and np.quantile(d, 0.999) <= 1e-5
    # [r4] one precision decision for the system (the ranks' votes are summed): every rank takes the single handle's
    # verdict - none turns all of its waves to float64 because ITS share is above one half (round 3: ranks 2 and 4
    # did).  The maximum over a million bodies is NOT the single handle's for all that (measured: 1.42e-5 against
    # 2.2e-6, the same 1.42e-5 as with the rank-local rule): which 64 bodies share a wave differs - a rank's waves
    # start at its first body, not at a multiple of 64 of the global order - and with it which bodies compute in
    # float64 and how the fp32 waves' sums associate; the body that ends worst after 100 steps of amplification is
    # another one.  Both stay well inside the bound; only force precision "f64" makes sharded == unsharded (1e-13,
    # test_owner_mode_walks_the_single_gpu_octree).
    all64 = [int(e.sim.force_precision_share()[1]) for e in engines]
    print(f"  single handle: max {single_err:.3e}, all-float64 {single_all64}; owner ranks all-float64 {all64}")
    assert all64 == [int(single_all64)] * world
    assert single_err <= 1e-4 and d.max() <= 10.0 * max(single_err, 2e-6)
    for r in range(1, world):
        assert np.array_equal(out[r][0], out[0][0])
    assert sum(e.sim.n for e in engines) == n
    for e in engines:
        e.sim.close()


def test_owner_mode_tree_export_repeats_when_its_launch_bound_was_too_small(gpu, monkeypatch):
    """nbmi_owner_export_let sizes its launches from the previous step's node count and repeats with the exact count
    when the header says the bound did not hold.  NBMI_LET_UNDERESTIMATE halves the bound, so every step from the
    second on takes the repeat path: results must not change."""
    from nbody.sharded import HipLetEngine, LetBarnesHut
    from tools.presets import generate_distribution
    np.random.seed(3)
    n, world, steps, dt = 40_003, 2, 4, 0.05
    pos, vel, mass = generate_distribution("galaxy", n, 500.0, 0.15)
    G, eps, theta = 0.15, 3.0, 0.5

    def run():
        comm = _ThreadComm(world)
        engines = [HipLetEngine(pos, vel, mass, G, eps, 1.0, theta, 0, r, world) for r in range(world)]
        steppers = [LetBarnesHut(e, r, world, comm.bind(r)) for r, e in enumerate(engines)]
        out = _run_ranks(steppers, comm, dt, steps)
        for e in engines:
            e.sim.close()
        return out[0][0]

    ref = run()
    monkeypatch.setenv("NBMI_LET_UNDERESTIMATE", "1")
    got = run()
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("zstd", [False, True])
def test_interrupt_inside_the_frame_write(gpu, tmp_path, monkeypatch, zstd):
    """Ctrl-C in the middle of a frame write: nothing of the frame may reach its name, the handler writes it
    (absolute, in a .zstd recording) together with the state, and the resumed recording equals the uninterrupted one."""
    from tools import record as rec
    from tools.presets import get_preset_config
    if zstd:
        try:
            rec._load_zstd()
        except RuntimeError:
            pytest.skip("no libzstd")
    cfg = get_preset_config("quick_galaxy")
    cfg.update(num_bodies=2000, theta=0.5, total_frames=8, substeps=2, zstd=zstd)
    whole = rec.record(dict(cfg, session_name="w_whole"), root=tmp_path, quiet=True, seed=12)
    real = rec._atomically
    calls = {"n": 0}

    def cut_short(path, write):
        if path.name.startswith("frame_"):
            calls["n"] += 1
            if calls["n"] == 4:  # frame 3: half of the bytes are written, then the interrupt arrives
                def half(f):
                    import io
                    buf = io.BytesIO()
                    write(buf)
                    f.write(buf.getvalue()[: len(buf.getvalue()) // 2])
                    f.flush()
                    raise KeyboardInterrupt
                return real(path, half)
        return real(path, write)

    monkeypatch.setattr(rec, "_atomically", cut_short)
    with pytest.raises(KeyboardInterrupt):
        rec.record(dict(cfg, session_name="w_cut"), root=tmp_path, quiet=True, seed=12)
    monkeypatch.setattr(rec, "_atomically", real)
    cut = tmp_path / "recordings" / "w_cut"
    assert not list(cut.glob(".*.part")), "a partial file was left behind"
    assert rec.get_completed_frames(cut) == 4 and (cut / "state_0003.npz").exists()
    a, _ = rec.load_frame(cut, 3)  # complete and readable
    b, _ = rec.load_frame(whole, 3)
    assert np.abs(a - b).max() <= (4e-3 if zstd else 1e-5)
    rec.record(dict(cfg, session_name="w_cut"), resume=True, root=tmp_path, quiet=True)
    assert rec.get_completed_frames(cut) == 8
    for k in range(8):
        a, _ = rec.load_frame(cut, k)
        b, _ = rec.load_frame(whole, k)
        assert np.abs(a - b).max() <= (4e-3 if zstd else 1e-5), k
