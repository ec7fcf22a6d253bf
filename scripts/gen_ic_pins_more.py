"""Writes two fixtures from the reference project:

  tests/golden/ic_pins_more.npz   the reference generate_distribution's "spiral" and "filament" arrays, in the layout
                                  of ic_pins.npz: sha256 of positions / velocities / masses, 64 head and 64 tail rows,
                                  params (R, G) - plus the seed, since one more seed than 42 is pinned
  tests/golden/presets_ref.json   the reference's 66 presets (settings only) and its preset-menu order

tests/test_presets_more_host.py checks tools.presets against both.

    python scripts/gen_ic_pins_more.py --reference <checkout of the reference project>

The reference's tools.presets is imported from that checkout at run time; nothing of it is copied.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
# (distribution, R, G) of a real preset: spiral_milkyway, cosmic_web
DISTS = [("spiral", 600.0, 0.08), ("filament", 1200.0, 0.02)]
SIZES = (256, 2048, 10_000, 100_000)
MORE = (7, 10_000)  # (seed, n) pinned besides seed 42


def tag(dist, n, seed):
    return f"{dist}_{n}" if seed == 42 else f"{dist}_{n}_s{seed}"


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("-o", "--output-dir", default=GOLDEN)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    from tools import presets as ref  # the reference's

    out = {}
    for dist, R, G in DISTS:
        for n, seed in [(n, 42) for n in SIZES] + [MORE[::-1]]:
            np.random.seed(seed)
            p, v, m = ref.generate_distribution(dist, n, R, G)
            t = tag(dist, n, seed)
            out[t + "_pos_sha"], out[t + "_vel_sha"], out[t + "_mass_sha"] = _sha(p), _sha(v), _sha(m)
            out[t + "_pos_head"], out[t + "_pos_tail"] = p[:64], p[-64:]
            out[t + "_vel_head"], out[t + "_vel_tail"] = v[:64], v[-64:]
            out[t + "_params"] = np.array([R, G])
            out[t + "_seed"] = np.int64(seed)
    path = os.path.join(a.output_dir, "ic_pins_more.npz")
    np.savez(path, **out)
    print(f"{path}: {len(out) // 9} pinned arrays")

    menu = [key for key, _ in ref.get_preset_list()]
    path = os.path.join(a.output_dir, "presets_ref.json")
    with open(path, "w") as f:
        json.dump({"presets": ref.PRESETS, "menu_order": menu}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(ref.PRESETS)} presets")


if __name__ == "__main__":
    main()
