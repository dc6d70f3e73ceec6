"""The fat-wave Gram matvec on v_mfma_f32_16x16x32_f16 (`k_rbf_fat_apply16`, csrc/mfx_rbf_fat.hip: RBF, d <= 8, 64-wide chunks;
MFX_RBF_FAT=2) against the fp64 HIP path of the same operator, with the 32x32x16 fat kernel (MFX_RBF_FAT=1) as the bar.

The bar: both kernels multiply the same 22-bit operands with the same chain folds, in a different order inside a tile, so their
errors against fp64 are one draw each from the same distribution.  The new kernel's error must be at most TWICE the old kernel's on
the same inputs; both figures are in the assertion message.  Where the new kernel does not take the shape (d > 8, <= 32 vectors)
or the f16 range guard sends the work to the fp32-distance launch, the result must be bit-identical to MFX_RBF_FAT=1.

The switches (MFX_RBF_FAT, MFX_RBF_SPLIT) are read once per process, so every configuration runs in one child process of its own,
once per module; the fp64 references are computed here.  Shapes: n = 8320 is 130 tiles -- with the column split forced to 1 a
workgroup crosses the chain fold at tile 128, with the natural split (15 ways at this n) it goes through k_split_reduce; n = 8257 is
ragged in rows and columns with the last tile partly empty.
"""

import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from matfree_extensions import _lib
    from matfree_extensions.operators import RbfGramOp

DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
RAW = (0.9, 0.4, -1.0)  # raw lengthscale, outputscale, noise

SHAPES = [(n, p, d) for n in (8320, 8257) for p in (33, 64, 65) for d in (1, 4, 5, 8)]
TILES = (0, 64, 129)  # first, middle, last tile of n = 8320


def _cases():
    """name -> (n, p, d, kind, row block or None)"""
    c = {f"shape-{n}-{p}-{d}": (n, p, d, "randn", None) for n, p, d in SHAPES}
    for d in (1, 4, 5, 8):
        c[f"unsplit-{d}"] = (8320, 64, d, "randn", None)
    c["rowblock"] = (8320, 64, 8, "randn", (1088, 700))
    for t in TILES:
        c[f"position-{t}"] = (8320, 64, 8, f"unit{t}", None)
    c["signs"] = (8320, 64, 8, "signs", None)
    c["scales"] = (8320, 64, 8, "scales", None)
    c["range"] = (8320, 64, 8, "range", None)
    c["dispatch-9-64"] = (8320, 64, 9, "randn", None)
    c["dispatch-16-64"] = (8320, 64, 16, "randn", None)
    c["dispatch-8-32"] = (8320, 32, 8, "randn", None)
    return c


NATURAL = [k for k in _cases() if not k.startswith("unsplit")]
UNSPLIT = [k for k in _cases() if k.startswith("unsplit")]


def _inputs(name):
    n, p, d, kind, block = _cases()[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    X = rng.standard_normal((n, d))
    if kind == "range":
        X *= 100.0  # |x|^2 ~ 8e4 > 6e4: k_pack_tiles raises the f16 range flag
    if kind.startswith("unit"):
        # a unit vector in each of the 64 columns of one tile: y[b] is column 64 tile + b of K, on every row tile of every wave
        V = np.zeros((p, n))
        V[np.arange(p), int(kind[4:]) * 64 + np.arange(p)] = 1.0
    elif kind == "signs":
        V = rng.choice([-1.0, 1.0], size=(p, n))  # lo halves exactly zero
    else:
        V = rng.standard_normal((p, n))
        if kind == "scales":
            V[0] *= 3e4  # per-vector power-of-two scales
            V[1] *= 3e-4
    return X, V, block


def _apply(X, V, dtype, block):
    Xt = torch.tensor(X, dtype=dtype, device=DEV)
    Vt = torch.tensor(V, dtype=dtype, device=DEV)
    op = RbfGramOp(Xt, noise_minval=1e-4)
    params = [torch.tensor(r, dtype=dtype, device=DEV) for r in RAW]
    with torch.no_grad():
        if block is None:
            y = op(Vt, *params)
        else:  # the row-sharded operator's path: rows [row0, row0 + nrows) of the product
            row0, nrows = block
            p, n = V.shape
            desc = op.descriptor(op.constrain(*params), Vt.dtype, n)
            desc.row0, desc.nrows = row0, nrows
            ws = _lib.workspace(desc, n, 1, p, Vt.device)
            y = torch.empty((p, nrows), dtype=dtype, device=DEV)
            _lib.check(_lib.get().mfx_op_apply(C.byref(desc), _lib.ptr(Vt), n, _lib.ptr(y), nrows, p, 0, _lib.ptr(ws), ws.numel(),
                                               _lib.stream_ptr(Vt.device)))
    return y.cpu().numpy()


def _run(names, out):
    """what a child process does: the fp32 operator on the named cases, under the switches of its environment"""
    res = {}
    for name in names:
        X, V, block = _inputs(name)
        res[name] = _apply(X, V, torch.float32, block)
    np.savez(out, **res)


CHILD = r"""
import sys
sys.path.insert(0, {tests!r})
sys.path.insert(0, {root!r})
sys.path.insert(0, {pkg!r})
import test_gpu_matvec_fat16 as t
t._run({names!r}, {out!r})
print("child ok")
"""


def _child(tmp, tag, names, **env_over):
    out = str(tmp / (tag + ".npz"))
    root = os.path.dirname(HERE)
    code = CHILD.format(tests=HERE, root=root, pkg=os.path.join(root, "experiments-lanczos-adjoints_amd"), names=names, out=out)
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, **env_over), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def new(tmp_path_factory):
    return _child(tmp_path_factory.mktemp("fat16"), "new", NATURAL, MFX_RBF_FAT="2")


@pytest.fixture(scope="module")
def old(tmp_path_factory):
    return _child(tmp_path_factory.mktemp("fat16"), "old", NATURAL, MFX_RBF_FAT="1")


@pytest.fixture(scope="module")
def new_unsplit(tmp_path_factory):
    return _child(tmp_path_factory.mktemp("fat16"), "new1", UNSPLIT, MFX_RBF_FAT="2", MFX_RBF_SPLIT="1")


@pytest.fixture(scope="module")
def old_unsplit(tmp_path_factory):
    return _child(tmp_path_factory.mktemp("fat16"), "old1", UNSPLIT, MFX_RBF_FAT="1", MFX_RBF_SPLIT="1")


_REF = {}


def _reference(name):
    if name not in _REF:
        X, V, block = _inputs(name)
        _REF[name] = _apply(X, V, torch.float64, block)
    return _REF[name]


def _err(y, ref, entrywise=False):
    e = np.abs(y.astype(np.float64) - ref)
    if entrywise:  # every entry against the oracle entry, in units of the largest one
        return e.max() / np.abs(ref).max()
    return (e.max(axis=1) / np.abs(ref).max(axis=1)).max()  # per vector, relative to its largest entry


def _at_most_twice(name, y_new, y_old, entrywise=False):
    ref = _reference(name)
    e_new, e_old = _err(y_new[name], ref, entrywise), _err(y_old[name], ref, entrywise)
    print(f"{name}: 16x16x32 {e_new:.3e}  32x32x16 {e_old:.3e}")
    assert np.isfinite(y_new[name]).all()
    assert e_new <= 2.0 * e_old, f"{name}: error against fp64 {e_new:.3e} (16x16x32) > 2 x {e_old:.3e} (32x32x16)"


@pytest.mark.parametrize("n,p,d", SHAPES)
def test_against_fp64_ragged_shapes_and_chunks(new, old, n, p, d):
    """130 tiles and a ragged n; 33, 64 and 65 vectors (65: two chunks, the second with one live vector); d across both padded
    dimensions.  At these n the dispatch splits the columns: gridDim.z > 1 and k_split_reduce."""
    _at_most_twice(f"shape-{n}-{p}-{d}", new, old)


@pytest.mark.parametrize("d", [1, 4, 5, 8])
def test_against_fp64_one_unsplit_sweep_across_a_chain_fold(new_unsplit, old_unsplit, d):
    """MFX_RBF_SPLIT=1: every workgroup sweeps all 130 tiles and folds its accumulators into the masters at tile 128."""
    _at_most_twice(f"unsplit-{d}", new_unsplit, old_unsplit)


def test_row_block_of_the_row_sharded_operator(new, old):
    """row0 = 1088 (a multiple of 64 inside a 512-row workgroup), 700 rows: ragged end inside a wave."""
    _at_most_twice("rowblock", new, old)


@pytest.mark.parametrize("tile", TILES)
def test_every_block_position_of_a_tile(new, old, tile):
    """A unit vector in each of the 64 columns of one tile picks out 64 columns of K on all rows: every (column, row tile, lane
    group) position of the unit pipeline, entry by entry against the oracle entry -- a misplaced entry is an O(1) error.
    The absolute bound guards against BOTH kernels being wrong: 3e-5 of the largest entry is the per-vector bound every split matvec
    of tests/test_gpu_matvec_kernels.py holds (the exponent, of size up to ~30 here, carries 2^-22 per product of the three-product
    split: ~1e-5 of an entry at worst); with a unit vector an entry's error IS the vector's."""
    _at_most_twice(f"position-{tile}", new, old, entrywise=True)
    ref = _reference(f"position-{tile}")
    assert np.abs(new[f"position-{tile}"] - ref).max() < 3e-5 * np.abs(ref).max()


@pytest.mark.parametrize("kind", ["signs", "scales"])
def test_probe_images_with_zero_lo_halves_and_per_vector_scales(new, old, kind):
    """probes of +-1 (the lo image is exactly zero); one vector scaled by 3e4 beside one scaled by 3e-4"""
    _at_most_twice(kind, new, old)


def test_f16_range_guard_hands_over_to_the_fp32_distance_launch(new, old):
    """|x|^2 > 6e4 raises the range flag: the fat kernels return at once and the fp32-distance launch does the work, as before.
    The two fat kernels never agree bit for bit on such a product, so equality shows that neither computed it.  (No bound against fp64
    here: at |x|^2 ~ 1e5 the fp32 distances themselves carry an error of ~1e-2 in the exponent, whichever kernel runs.)"""
    assert np.isfinite(new["range"]).all()
    assert np.array_equal(new["range"], old["range"])
    assert not np.array_equal(new["shape-8320-64-8"], old["shape-8320-64-8"])


@pytest.mark.parametrize("d,p", [(9, 64), (16, 64), (8, 32)])
def test_shapes_the_new_kernel_does_not_take_are_bit_identical(new, old, d, p):
    """d > 8 and chunks of at most 32 vectors stay on k_rbf_fat_apply under MFX_RBF_FAT=2"""
    name = f"dispatch-{d}-{p}"
    assert np.array_equal(new[name], old[name])
    assert _err(new[name], _reference(name)) < 3e-5
