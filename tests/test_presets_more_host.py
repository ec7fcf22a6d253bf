"""Host side of the spiral / cosmic-web presets: the two new generators against the reference's arrays
(tests/golden/ic_pins_more.npz), the preset table against the reference's (presets_ref.json), and the
`python -m tools.record` command line up to the point where it would start the GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

PINS = [(dist, n, 42) for dist in ("spiral", "filament") for n in (256, 2048, 10_000, 100_000)] + \
       [("spiral", 10_000, 7), ("filament", 10_000, 7)]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _ref_presets():
    with open(os.path.join(GOLDEN, "presets_ref.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("dist,n,seed", PINS)
def test_spiral_and_filament_match_reference(dist, n, seed):
    from tools.presets import generate_distribution
    g = golden("ic_pins_more")
    t = f"{dist}_{n}" if seed == 42 else f"{dist}_{n}_s{seed}"
    assert int(g[t + "_seed"]) == seed
    R, G = g[t + "_params"]
    np.random.seed(seed)
    p, v, m = generate_distribution(dist, n, float(R), float(G))
    assert p.dtype == v.dtype == m.dtype == np.float64 and p.shape == v.shape == (n, 3) and m.shape == (n,)
    assert np.array_equal(p[:64], g[t + "_pos_head"]) and np.array_equal(p[-64:], g[t + "_pos_tail"])
    assert np.array_equal(v[:64], g[t + "_vel_head"]) and np.array_equal(v[-64:], g[t + "_vel_tail"])
    assert _sha(p) == str(g[t + "_pos_sha"]) and _sha(v) == str(g[t + "_vel_sha"])
    assert _sha(m) == str(g[t + "_mass_sha"])


def test_filament_masses_and_spiral_com():
    from tools.presets import generate_distribution
    np.random.seed(3)
    _, _, m = generate_distribution("filament", 500, 1200.0, 0.02)
    assert np.all(m == 0.1)
    np.random.seed(3)
    _, v, m = generate_distribution("spiral", 500, 600.0, 0.08)
    assert np.all(m == 1.0) and np.abs(v.mean(axis=0)).max() < 1e-9


def test_unknown_distributions_still_raise():
    from tools.presets import DISTRIBUTIONS, generate_distribution
    assert sorted(DISTRIBUTIONS) == ["cluster", "collision", "filament", "galaxy", "spiral"]
    for name in ("torus", "ring", "vortex", ""):
        with pytest.raises(ValueError):
            generate_distribution(name, 10, 1.0, 1.0)


def test_presets_equal_reference_entries():
    from tools.presets import DISTRIBUTIONS, PRESETS
    ref = _ref_presets()["presets"]
    assert len(ref) == 66
    want = {k for k, v in ref.items() if v["distribution"] in DISTRIBUTIONS}
    assert set(PRESETS) == want and len(want) == 35
    for key, p in PRESETS.items():
        assert p == ref[key], key
        for field, value in p.items():  # 1 vs 1.0 would survive ==, not JSON round trips of metadata.json
            assert type(value) is type(ref[key][field]), (key, field)
    by_dist = {}
    for p in PRESETS.values():
        by_dist[p["distribution"]] = by_dist.get(p["distribution"], 0) + 1
    assert by_dist == {"galaxy": 11, "collision": 10, "cluster": 4, "spiral": 5, "filament": 5}


def test_preset_list_follows_reference_order():
    from tools.presets import PRESETS, get_preset_by_index, get_preset_list
    ref = _ref_presets()["menu_order"]
    mine = [k for k, _ in get_preset_list()]
    assert mine == [k for k in ref if k in PRESETS]
    assert get_preset_by_index(0) == get_preset_list()[0]
    assert get_preset_by_index(len(PRESETS)) == (None, None) and get_preset_by_index(-1) == (None, None)


def test_existing_presets_unchanged():
    from tools.presets import get_preset_config
    c = get_preset_config("quick_galaxy")
    assert c["session_name"] == "quick_galaxy" and c["num_bodies"] == 100_000 and c["distribution"] == "galaxy"
    assert get_preset_config("extreme_50m_web")["num_bodies"] == 50_000_000
    assert get_preset_config("nope") is None


def test_list_distributions(capsys):
    from tools.presets import list_distributions
    list_distributions()
    out = capsys.readouterr().out
    assert "spiral" in out and "filament" in out and "torus" not in out


# ---- command line ---------------------------------------------------------------------------------------------
def _config(argv):
    from tools.record import build_config, build_parser
    return build_config(build_parser().parse_args(argv))


def test_cli_config_overrides():
    from tools.presets import get_preset_config
    c = _config(["--preset", "cosmic_web", "-n", "1.5m", "-f", "12", "-t", "0.7", "--dt", "0.05"])
    base = get_preset_config("cosmic_web")
    assert c["num_bodies"] == 1_500_000 and c["total_frames"] == 12 and c["theta"] == 0.7
    assert c["dt_per_frame"] == 0.05 and "dt" not in c  # --dt sets dt_per_frame here
    changed = ("num_bodies", "total_frames", "theta", "dt_per_frame")
    assert {k: v for k, v in c.items() if k not in changed} == {k: v for k, v in base.items() if k not in changed}
    assert _config(["--preset", "quick_galaxy", "-n", "20k"])["num_bodies"] == 20_000
    assert _config(["--preset", "quick_galaxy", "--bodies", "12345"])["num_bodies"] == 12_345
    assert _config(["my_run", "--preset", "quick_galaxy"])["session_name"] == "my_run"
    assert "device_ic" not in _config(["--preset", "quick_galaxy"])
    with pytest.raises(ValueError, match="Invalid bodies"):
        _config(["--preset", "quick_galaxy", "-n", "lots"])


def test_cli_preset_id_indexes_this_builds_list():
    from tools.presets import get_preset_list
    for idx in (0, 7, len(get_preset_list()) - 1):
        assert _config(["--preset-id", str(idx)])["session_name"] == get_preset_list()[idx][0]
    with pytest.raises(ValueError, match="Invalid preset index"):
        _config(["--preset-id", "35"])


def test_cli_unknown_preset_fails_and_writes_nothing(tmp_path, capsys):
    from tools.record import main
    assert main(["--preset", "no_such_preset", "--root", str(tmp_path)]) != 0
    assert main(["--preset-id", "99", "--root", str(tmp_path)]) != 0
    assert main(["--root", str(tmp_path)]) != 0  # no interactive menu in this build
    assert list(tmp_path.iterdir()) == []
    assert "Unknown preset" in capsys.readouterr().out


def test_cli_device_ic_needs_a_device_generator(tmp_path, monkeypatch):
    from tools import presets
    from tools.record import main
    for dist in ("galaxy", "collision", "cluster", "spiral", "filament"):
        key = next(k for k, p in presets.PRESETS.items() if p["distribution"] == dist)
        assert _config(["--preset", key, "--device-ic"])["device_ic"] is True
    assert _config(["--preset", "demo_cluster", "--device-ic", "-n", "1k"])["num_bodies"] == 1000
    # a preset built on a distribution without a device generator is rejected before any GPU work
    monkeypatch.setitem(presets.PRESETS, "host_only", dict(presets.PRESETS["tiny_galaxy"], distribution="torus"))
    with pytest.raises(ValueError, match="no device generator"):
        _config(["--preset", "host_only", "--device-ic"])
    assert main(["--preset", "host_only", "--device-ic", "--root", str(tmp_path)]) != 0
    assert list(tmp_path.iterdir()) == []


def _fake_session(root, name, total, frames, **extra):
    from tools.record import save_frame, save_metadata
    d = root / "recordings" / name
    d.mkdir(parents=True)
    cfg = {"num_bodies": 8, "theta": 0.9, "distribution": "filament", "total_frames": total, **extra}
    save_metadata(d, cfg, 1_700_000_000.0)
    for k in range(frames):
        save_frame(d, k, np.zeros((8, 3)), np.ones((8, 3)))
    return d


def test_cli_list_and_status(tmp_path, capsys):
    from tools.record import main
    _fake_session(tmp_path, "web_a", 4, 4)
    _fake_session(tmp_path, "web_b", 10, 3)
    (tmp_path / "recordings" / "not_a_session").mkdir()
    assert main(["--list", "--root", str(tmp_path)]) == 0
    out = capsys.readouterr().out
    assert "Found 2 recording(s)" in out and "not_a_session" not in out
    lines = {ln.split("|")[0].strip(): ln for ln in out.splitlines() if "|" in ln}
    assert "4/4" in lines["web_a"] and "done" in lines["web_a"]
    assert "3/10" in lines["web_b"] and "30%" in lines["web_b"]
    assert main(["web_b", "--status", "--root", str(tmp_path)]) == 0
    out = capsys.readouterr().out
    assert "Progress: 3/10 frames (30.0%)" in out and "Distribution: filament" in out and "--resume web_b" in out
    assert main(["missing", "--status", "--root", str(tmp_path)]) != 0
    assert not (tmp_path / "recordings" / "missing").exists()
    assert main(["--status", "--root", str(tmp_path)]) == 0  # no session: the list
    assert "Found 2 recording(s)" in capsys.readouterr().out
    empty = tmp_path / "empty"
    assert main(["--list", "--root", str(empty)]) == 0 and "No recordings found" in capsys.readouterr().out


def test_cli_resume_and_extend_without_a_session_fail_cleanly(tmp_path):
    from tools.record import main
    assert main(["--resume", "--root", str(tmp_path)]) != 0
    assert main(["ghost", "--resume", "--root", str(tmp_path)]) != 0
    assert main(["--extend", "5", "--root", str(tmp_path)]) != 0
    assert main(["ghost", "--extend", "5", "--root", str(tmp_path)]) != 0
    assert not (tmp_path / "recordings" / "ghost").exists()


def test_parse_number():
    from tools.record import parse_number
    assert parse_number("1.5m") == 1_500_000 and parse_number("100K") == 100_000 and parse_number(" 42 ") == 42
    with pytest.raises(ValueError):
        parse_number("1.5x")
