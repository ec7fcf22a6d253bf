"""Host half of the leapfrog integrator: the float64 reference schemes the GPU tests compare against,
the C-ABI names, the Python refusals that need no device and the recorder's CLI / metadata round trip."""
import json
import re
import os

import numpy as np
import pytest

import leapfrog_ref as lf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_kepler_orders():
    """Quarter period of the circular pair at T/200 and T/400: leapfrog's errors shrink 4x, kick-drift's 2x."""
    x0, v0, m = lf.kepler_pair()
    force = lf.direct_force(1.0, 0.0)
    xe, ve = lf.kepler_exact(np.pi / 2)
    err = {"lf": [], "kd": []}
    for steps in (50, 100):
        dt = np.pi / 2 / steps
        x, v, _ = lf.leapfrog(x0, v0, m, force, dt, steps)
        err["lf"].append((np.abs(x - xe).max(), np.abs(v - ve).max()))
        x, v = lf.kick_drift(x0, v0, m, force, dt, steps)
        err["kd"].append((np.abs(x - xe).max(), np.abs(v - ve).max()))
    for k in range(2):
        assert 3.5 <= err["lf"][0][k] / err["lf"][1][k] <= 4.5
        assert err["kd"][0][k] / err["kd"][1][k] < 2.5


def test_reference_leapfrog_is_reversible():
    x0, v0, m = lf.plummer(64, 2)
    force = lf.direct_force(1.0, 0.05)
    x, v, _ = lf.leapfrog(x0, v0, m, force, 0.01, 50)
    x, v, _ = lf.leapfrog(x, -v, m, force, 0.01, 50)
    assert np.abs(x - x0).max() <= 1e-12 * np.abs(x0).max()
    assert np.abs(v + v0).max() <= 1e-12 * np.abs(v0).max()
    x, v = lf.kick_drift(x0, v0, m, force, 0.01, 50)
    x, v = lf.kick_drift(x, -v, m, force, 0.01, 50)
    assert np.abs(x - x0).max() > 1e-6 * np.abs(x0).max()


def test_plummer_sphere_and_kepler_setup():
    x, v, m = lf.plummer(512, 3)
    assert x.shape == (512, 3) and abs(m.sum() - 1.0) < 0.05 and np.abs(x).max() <= 10.0 * np.sqrt(3.0)
    assert np.abs((m[:, None] * x).sum(0)).max() < 1e-12 and np.abs((m[:, None] * v).sum(0)).max() < 1e-12
    assert m.min() >= 0.5 / 512 and m.max() <= 1.5 / 512
    kx, kv, km = lf.kepler_pair()
    ex, ev = lf.kepler_exact(0.0)
    assert np.array_equal(kx, ex) and np.allclose(kv, ev)
    # circular: the pull of the partner equals v^2 / r
    a = lf.direct_force(1.0, 0.0)(kx, km)
    assert np.allclose(np.linalg.norm(a, axis=1), 0.25 / 0.5)


def test_integrator_codes_match_the_header():
    import nbmi_native
    from nbody.gpu_backend import INTEGRATORS
    hdr = open(os.path.join(ROOT, "include", "nbmi.h")).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define NBMI_INTEGRATOR_(\w+) (\d+)", hdr)}
    assert codes == INTEGRATORS == {"kick_drift": 0, "leapfrog": 1}
    for name in ("nbmi_set_integrator", "nbmi_get_integrator"):
        assert name in nbmi_native.PROTOTYPES and re.search(r"\b%s\(" % name, hdr)


def test_python_refusals_without_a_device():
    from nbody import gpu_backend as gb
    from nbody import sharded
    with pytest.raises(ValueError, match="integrator must be one of"):
        gb._integrator_code("verlet")
    x = np.zeros((4, 3))
    with pytest.raises(ValueError, match="kick_drift"):
        sharded.create_sharded_simulation(x, x, np.ones(4), 1.0, 0.1, 1.0, integrator="leapfrog")
    with pytest.raises(ValueError, match="kick_drift"):
        sharded.HipShardEngine(x, x, np.ones(4), 1.0, 0.1, 1.0, 0.5, 0, integrator="leapfrog")
    with pytest.raises(ValueError, match="kick_drift"):
        sharded.HipLetEngine(x, x, np.ones(4), 1.0, 0.1, 1.0, 0.5, 0, 0, 1, integrator="leapfrog")


def test_record_cli_and_metadata_round_trip(tmp_path, capsys):
    from tools import record as rec
    ap = rec.build_parser()
    cfg = rec.build_config(ap.parse_args(["--preset", "quick_galaxy", "--integrator", "leapfrog"]))
    assert cfg["integrator"] == "leapfrog"
    for argv in ([], ["--integrator", "kick_drift"]):
        assert "integrator" not in rec.build_config(ap.parse_args(["--preset", "quick_galaxy"] + argv))
    with pytest.raises(SystemExit):
        ap.parse_args(["--preset", "quick_galaxy", "--integrator", "verlet"])
    capsys.readouterr()
    for name, c in (("lf", cfg), ("plain", rec.build_config(ap.parse_args(["--preset", "quick_galaxy"])))):
        d = tmp_path / "recordings" / name
        d.mkdir(parents=True)
        rec.save_metadata(d, dict(c, session_name=name), 0.0)
        meta = json.loads((d / "metadata.json").read_text())
        assert meta.get("integrator") == ("leapfrog" if name == "lf" else None)
        assert rec.show_status(name, root=tmp_path)
        out = capsys.readouterr().out
        assert ("Integrator: leapfrog" if name == "lf" else "Integrator: kick_drift") in out
