"""Bit-identity of two builds of the Gram matvec kernel `k_rbf_fat_apply16` (same products, same order, same accumulators):
    python tools/fat16_bit_identity.py <reference libmfx.so> <candidate libmfx.so> [<bench dump dir of the reference> <of the candidate>]
Runs every case of tests/test_gpu_matvec_fat16_tiles.py (MFX_RBF_FAT=2; column split 1 and the natural split) once per library, each in
a child process of its own (MFX_LIBRARY_PATH is read at import), and compares the outputs with numpy.array_equal; then, if given, the
arrays two `bench.py --steps 1 --warmup 0 --dump-outputs DIR` runs wrote.  Prints one line per array and exits 1 on any difference."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r"""
import sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r}); sys.path.insert(0, {pkg!r})
import test_gpu_matvec_fat16_tiles as t
t._run(t.CASES, {out!r})
print("child ok")
"""


def outputs(lib, split, tmp):
    out = os.path.join(tmp, f"{abs(hash(lib))}_{split}.npz")
    env = dict(os.environ, MFX_LIBRARY_PATH=os.path.abspath(lib), MFX_RBF_FAT="2")
    if split != "natural":
        env["MFX_RBF_SPLIT"] = split
    code = CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT, pkg=os.path.join(ROOT, "experiments-lanczos-adjoints_amd"), out=out)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(np.load(out))


def main():
    ref, cand = sys.argv[1:3]
    bad = total = 0
    with tempfile.TemporaryDirectory() as tmp:
        for split in ("1", "natural"):
            a, b = outputs(ref, split, tmp), outputs(cand, split, tmp)
            assert sorted(a) == sorted(b)
            for name in sorted(a):
                same = bool(np.array_equal(a[name], b[name]))
                total += 1
                bad += not same
                print(f"split {split:8s} {name:18s} shape {a[name].shape}  array_equal {same}")
    if len(sys.argv) >= 5:
        da, db = sys.argv[3:5]
        names = sorted(f for f in os.listdir(da) if f.endswith(".npy"))
        assert names and names == sorted(f for f in os.listdir(db) if f.endswith(".npy")), (names, os.listdir(db))
        for f in names:
            x, y = np.load(os.path.join(da, f)), np.load(os.path.join(db, f))
            same = bool(np.array_equal(x, y))
            total += 1
            bad += not same
            print(f"bench.py --dump-outputs {f:24s} shape {x.shape} dtype {x.dtype}  array_equal {same}")
    print(f"{total - bad} of {total} arrays bit-identical: reference {ref}, candidate {cand}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
