"""The tile loop of `k_rbf_fat_apply16` (csrc/mfx_rbf_fat.hip; MFX_RBF_FAT=2) at every tile count at which it takes another path.

The loop runs two 64-column tiles per iteration (one per LDS buffer), peels the last tile of an odd count, and folds the
accumulators into the chain masters between chains of kChainTiles = 128 tiles (8192 columns).  The shapes are the smallest at which
each of these can go wrong:

  * tile parity and the peeled tile:  n = 512, 576, 640, 704            (8, 9, 10, 11 tiles)
  * ragged last tile:                 n = 513, 609, 703                  (9, 10, 11 tiles, the last with 1, 33, 63 live columns)
  * a fold in front of the peeled tile, of a loop body, of the second chain's end:
                                      n = 8256, 8320, 16448, 16576, 16481 (129, 130, 257, 259, 258 tiles; the last ragged)

each at d = 1, 5, 8 (different k-fill of the distance product) with 64 vectors, once with random vectors and once with unit vectors
that put a single non-zero in the first and in the last column of the tiles around every such boundary and in the column before a
fold: a dropped, doubled or misplaced tile is then an O(1) error of an entry, not noise.

One workgroup sweeps all tiles only when the column split is 1, so every case runs twice: with MFX_RBF_SPLIT=1 (the tile counts above)
and with the natural split (the same n in up to 16 column ranges of 8 to 17 tiles: further parities, and the partial sums).

Reference and bar are those of tests/test_gpu_matvec_fat16.py: the fp64 HIP path of the same operator is the reference, the 32x32x16
kernel (MFX_RBF_FAT=1) the yardstick; against fp64 the 16x16x32 kernel's error may be at most TWICE the yardstick's on the same
inputs.  The switches are read once per process, so every configuration runs in one child process of its own, once per module.
"""

import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions.operators import RbfGramOp

DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
RAW = (0.9, 0.4, -1.0)  # raw lengthscale, outputscale, noise
P = 64
FOLD = 8192  # kChainTiles * 64 columns

PARITY = (512, 576, 640, 704)
RAGGED = (512 + 1, 576 + 33, 640 + 63)
FOLDS = (8192 + 64, 8192 + 128, 16384 + 64, 16384 + 192, 16384 + 97)
NS = PARITY + RAGGED + FOLDS
DS = (1, 5, 8)
KINDS = ("randn", "unit")
CASES = [f"{kind}-{n}-{d}" for n in NS for d in DS for kind in KINDS]


def unit_columns(n):
    """The 64 columns of the unit vectors: first and last column of the tiles at the start and the end of the sweep and on both sides
    of every fold, the column before each fold, and (to fill up) the first columns of further tiles."""
    ntile = (n + 63) // 64
    tiles = [0, 1, 2, ntile - 3, ntile - 2, ntile - 1]
    for f in range(128, ntile + 1, 128):
        tiles += [f - 2, f - 1, f, f + 1]
    cols = [f * 64 - 1 for f in range(128, ntile + 1, 128) if f * 64 - 1 < n]  # the column before a fold
    for t in tiles:
        if 0 <= t < ntile:
            cols += [64 * t, min(64 * t + 63, n - 1)]
    cols += [64 * (t % ntile) + t // ntile for t in range(3, 3 + 64 * ntile)]  # first, then second, ... columns of the other tiles
    seen, out = set(), []
    for c in cols:
        if c not in seen and c < n:
            seen.add(c)
            out.append(c)
    return np.array(out[:P])


def _inputs(name):
    kind, n, d = name.split("-")
    n, d = int(n), int(d)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    X = rng.standard_normal((n, d))
    if kind == "unit":
        V = np.zeros((P, n))
        V[np.arange(P), unit_columns(n)] = 1.0
    else:
        V = rng.standard_normal((P, n))
    return X, V


def _apply(X, V, dtype):
    Xt = torch.tensor(X, dtype=dtype, device=DEV)
    Vt = torch.tensor(V, dtype=dtype, device=DEV)
    op = RbfGramOp(Xt, noise_minval=1e-4)
    params = [torch.tensor(r, dtype=dtype, device=DEV) for r in RAW]
    with torch.no_grad():
        y = op(Vt, *params)
    return y.cpu().numpy()


def _run(names, out):
    """what a child process does: the fp32 operator on the named cases, under the switches of its environment"""
    np.savez(out, **{name: _apply(*_inputs(name), torch.float32) for name in names})


CHILD = r"""
import sys
sys.path.insert(0, {tests!r})
sys.path.insert(0, {root!r})
sys.path.insert(0, {pkg!r})
import test_gpu_matvec_fat16_tiles as t
t._run({names!r}, {out!r})
print("child ok")
"""


def _child(tmp, tag, **env_over):
    out = str(tmp / (tag + ".npz"))
    root = os.path.dirname(HERE)
    code = CHILD.format(tests=HERE, root=root, pkg=os.path.join(root, "experiments-lanczos-adjoints_amd"), names=CASES, out=out)
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, **env_over), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """(split, kernel) -> outputs of every case; split "1": one workgroup sweeps all tiles, "natural": the dispatch's own split"""
    tmp = tmp_path_factory.mktemp("fat16_tiles")
    res = {}
    for split, env in (("1", {"MFX_RBF_SPLIT": "1"}), ("natural", {})):
        for fat in ("2", "1"):
            res[split, fat] = _child(tmp, f"fat{fat}_split{split}", MFX_RBF_FAT=fat, **env)
    return res


_REF = {}


def _reference(name):
    if name not in _REF:
        _REF[name] = _apply(*_inputs(name), torch.float64)
    return _REF[name]


def _err(y, ref, entrywise):
    e = np.abs(y.astype(np.float64) - ref)
    if entrywise:  # every entry against the oracle entry, in units of the largest one
        return e.max() / np.abs(ref).max()
    return (e.max(axis=1) / np.abs(ref).max(axis=1)).max()  # per vector, relative to its largest entry


def _at_most_twice(results, split, name):
    ref = _reference(name)
    entrywise = name.startswith("unit")
    y_new, y_old = results[split, "2"][name], results[split, "1"][name]
    e_new, e_old = _err(y_new, ref, entrywise), _err(y_old, ref, entrywise)
    print(f"{name} split {split}: 16x16x32 {e_new:.3e}  32x32x16 {e_old:.3e}")
    assert y_new.shape == ref.shape and np.isfinite(y_new).all()
    assert e_new <= 2.0 * e_old, f"{name} split {split}: error against fp64 {e_new:.3e} (16x16x32) > 2 x {e_old:.3e} (32x32x16)"


def test_unit_vectors_sit_on_the_tile_and_fold_boundaries():
    """the input construction itself: 64 distinct columns, among them the first and last column of the first, the last and the peeled
    tile, both sides of every fold and the column before it"""
    for n in NS:
        cols = unit_columns(n)
        ntile = (n + 63) // 64
        assert len(set(cols.tolist())) == P and cols.min() == 0 and cols.max() == n - 1
        assert {0, 63, 64, 127, 64 * (ntile - 1), 64 * (ntile - 2), 64 * (ntile - 2) + 63} <= set(cols.tolist())
        for f in range(FOLD, n, FOLD):
            assert {f - 64, f - 1, f, min(f + 63, n - 1)} <= set(cols.tolist())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", PARITY)
@pytest.mark.parametrize("split", ["1", "natural"])
def test_tile_parity_and_the_peeled_tile(results, split, n, d, kind):
    """8 and 10 tiles: whole loop bodies; 9 and 11: the last tile is peeled"""
    _at_most_twice(results, split, f"{kind}-{n}-{d}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", RAGGED)
@pytest.mark.parametrize("split", ["1", "natural"])
def test_ragged_last_tile(results, split, n, d, kind):
    """the last tile holds 1 live column (peeled), 33 (second half of a loop body) and 63 (peeled)"""
    _at_most_twice(results, split, f"{kind}-{n}-{d}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", FOLDS)
@pytest.mark.parametrize("split", ["1", "natural"])
def test_chain_fold_before_a_loop_body_and_before_the_peeled_tile(results, split, n, d, kind):
    """129 tiles: the fold at tile 128 stands in front of the peeled tile; 130: in front of a loop body; 257, 259: a second fold, again
    before the peeled tile and before a body; 258 tiles with a ragged last one"""
    _at_most_twice(results, split, f"{kind}-{n}-{d}")
