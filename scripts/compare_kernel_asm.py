"""Are the kernels of one file of csrc/ the same instructions in two source trees?  (the walled, noise-free
sweep against the commit before the periodic box; 4.20: the state sums against the commit before their shared pieces.)
Needs hipcc and c++filt, no GPU.

    git worktree add /tmp/parent <commit>
    python scripts/compare_kernel_asm.py [--file nbmi.hip] [--pair OLD=NEW ...] /tmp/parent . [kernel name fragments ...]

Each tree's file (bdmi.hip unless --file names another) is compiled to device assembly for gfx950 with the Makefile's
flags.  --pair compares kernel OLD of the first tree with kernel NEW of the second, both written as this script prints
names (--pair 'k_deposit_max=k_plane_max<6, DepSource>').  Otherwise kernels are matched by their
demangled name up to the argument list, with the template arguments this tree added for the walled, noise-free instances
(", GridP, FlockP" / ", GridP" / ", FsBox" / "<GridP>") dropped, so k_flock<true> of the old tree meets
k_flock<true, GridP, FlockP> of the new one, k_fs_link meets k_fs_link<GridP> and k_fs_chunks<1> meets k_fs_chunks<1, FsBox>.  Compared: the instruction lines, with symbol names and block labels normalised, and the register, LDS and scratch
figures of the kernel descriptor.  Exit status 1 if a kernel present in both trees differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

PKG = "3d-spatial-sim-for-boid-and-nbody_amd"
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S"]
FACTS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")
ANON = "(anonymous namespace)::"


def kernels(tree, tmp, tag, file):
    out = os.path.join(tmp, tag + ".s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, *FLAGS, "-o", out, os.path.join(tree, PKG, "csrc", file)], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {m.group(1): m.group(2)
             for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)}
    names = subprocess.run(["c++filt", *found], capture_output=True, text=True, check=True).stdout.split("\n")
    res = {}
    for name, body in zip(names, found.values()):
        short = name.replace(ANON, "").split("(")[0]
        short = short[5:] if short.startswith("void ") else short  # a template instance carries its return type
        for added in ((", GridP, FlockP>", ">"), (", GridP>", ">"), (", FsBox>", ">"), ("<GridP>", "")):
            short = short.replace(*added)
        res[short] = body
    return res


def instructions(body):
    lines = []
    for line in body.split("\n"):
        line = line.split(";")[0].rstrip()
        if line.strip() and not line.lstrip().startswith("."):
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", line)))
    return lines


def facts(body):
    return tuple(int(re.search(r"\.amdhsa_" + k + r"\s+(\d+)", body).group(1)) for k in FACTS)


def main(argv):
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("--file", default="bdmi.hip")
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("trees", nargs=2)
    ap.add_argument("fragments", nargs="*")
    opt = ap.parse_args(argv)
    argv = opt.trees + opt.fragments
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernels(argv[0], tmp, "a", opt.file), kernels(argv[1], tmp, "b", opt.file)
    for old, new in (p.split("=", 1) for p in opt.pair):
        if old not in a or new not in b:
            raise SystemExit(f"--pair {old}={new}: no kernel {old} in {argv[0]} or no {new} in {argv[1]}")
        a[new] = a.pop(old)
    differ = 0
    for name in sorted(set(a) & set(b)):
        if argv[2:] and not any(f in name for f in argv[2:]):
            continue
        ia, ib = instructions(a[name]), instructions(b[name])
        moved = sum(x != y for x, y in zip(ia, ib)) + abs(len(ia) - len(ib))
        same = ia == ib and facts(a[name]) == facts(b[name])
        differ += not same
        print(f"{'identical' if same else 'DIFFERS  '} {name}: {len(ia)} / {len(ib)} instructions"
              + ("" if same else f", {moved} lines differ") + f", vgpr/sgpr/lds/scratch {facts(a[name])} / {facts(b[name])}")
    only = sorted(set(b) - set(a))
    print(f"{len(only)} kernels only in {argv[1]}:", ", ".join(only))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
