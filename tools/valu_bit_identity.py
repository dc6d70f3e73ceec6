"""Two builds of libmfx.so on the VALU kernel-Gram kernels of csrc/mfx_rbf_valu.hip: the same bits, and the same speed?
    python tools/valu_bit_identity.py <reference libmfx.so> <candidate libmfx.so>            # every array compared with numpy.array_equal
    python tools/valu_bit_identity.py <reference libmfx.so> <candidate libmfx.so> --time     # device-event medians of the sweeps
Each library runs in a child process of its own (MFX_LIBRARY_PATH is read at import), one after the other.  The sweeps use no atomics
and a fixed order of sums, so two builds that differ only in how the source is laid out give the same bits; exit status 1 on any
difference.

Bit cases: fp64 and fp32; d in {3, 12, 24, 40, 70} (padded 4, 12, 32; wide with 2 and 3 selections); scalar and ARD lengthscale; RBF
and Matern-3/2; (n, m, batch) in {(300, 70, 40), (300, 300, 1), (5, 70, 1)}: n = 300 is a second, partial workgroup and a tail tile
at every tile width (8, 16, 32, 64, 128), n = 5 fewer columns than any tile, m = 70 a workgroup with dead waves, batch = 40 a second,
partial staging chunk of the factored weights.  Entry points, with the kernel each reaches:
  matvec, whole operator and the row block [37, 237)   k_rbf_apply[_wide]; fp64 p = 1, 2, 3, 8, fp32 p = 1, 2, 3 (fp32 stays on the
                                                       VALU for p < 4 and n < 2048: rbf_apply_path)
  parameter VJP, whole operator and the row block      k_rbf_grad[_wide] + k_rbf_grad_final; not fp32 with n = 300, batch = 40 and
                                                       d <= 64, which takes the matrix-core sweep (rbf_grad_path)
  input VJP                                            k_rbf_grad_x[_wide]
  cross matvec and its transpose, p = 1 and 3          k_rbf_apply[_wide], row0 = -1
  factored cross VJP: theta, X_new, X, all three       k_rbf_cross_grad[_wide]<FactoredSrc> (+ k_rbf_cross_gx_final, k_rbf_grad_final)
  dense cross VJP, lds = n (16-byte loads) and n + 1   k_rbf_cross_grad[_wide]<DenseSrc>
  Gram block, symmetric (m x m) and m x n              k_gram_block[_wide]
One of the m points equals a training point (a clamped pair).

--time: parameter VJP, input VJP and factored cross VJP (m = 1024 owners, every gradient) at n = 8192, batch = 16, d = 8 and 40, in fp64
and -- the input and cross sweeps, which have no matrix-core form -- in fp32; the fp32 parameter sweep of these shapes runs on the
matrix cores and is left out.  Runs reference, candidate, reference, candidate; prints each run's median of --reps repeats, the
reference's own difference between its two runs (the margin), and the candidate's median against the reference's."""
import argparse
import ctypes as C
import itertools
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((300, 70, 40), (300, 300, 1), (5, 70, 1))  # n, m, batch
DIMS = (3, 12, 24, 40, 70)
ROW0, NROWS = 37, 200  # the row block (n = 300 only)


def grad_path(f32, d, n, batch):
    """rbf_grad_path of csrc/mfx_rbf_mfma_grad.hip"""
    return "mfma" if f32 and d <= 64 and n >= 256 and (batch >= 16 or n >= 2048) else "valu"


def setup(dtype, n, m, d, ard, kind, batch, seed):
    import torch
    from matfree_extensions.operators import RbfGramOp

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g, dtype=dtype)  # noqa: E731
    X, xnew = rnd(n, d) / (d / 4) ** 0.5, rnd(m, d) / (d / 4) ** 0.5
    xnew[0] = X[min(5, n - 1)]
    raw = (torch.linspace(-0.3, 0.4, d, device=dev, dtype=dtype) if ard else torch.tensor(0.2, device=dev, dtype=dtype),
           torch.tensor(0.1, device=dev, dtype=dtype), torch.tensor(-1.0, device=dev, dtype=dtype))
    op = RbfGramOp(X, kernel=kind, precision="fp32")
    cparams = op.constrain(*raw)
    return dev, rnd, X, xnew, cparams, op.descriptor(cparams, dtype, n)


def new_grads(cparams, n, m, d, theta, x, noise=False):
    import torch
    from matfree_extensions import _lib

    dtype, dev = cparams[0].dtype, cparams[0].device
    o = {"ls": torch.zeros_like(cparams[0]), "s": torch.zeros_like(cparams[1]), "noise": torch.zeros_like(cparams[2]),
         "X": torch.zeros(n, d, dtype=dtype, device=dev), "xnew": torch.zeros(m, d, dtype=dtype, device=dev)}
    st = _lib.OpGrads()
    if theta:
        st.lengthscale, st.outputscale = o["ls"].data_ptr(), o["s"].data_ptr()
    if noise:
        st.noise = o["noise"].data_ptr()
    if x:
        st.x = o["X"].data_ptr()
    return o, st


def child_bits(path):
    import torch
    from matfree_extensions import _lib

    lib, out = _lib.get(), {}
    for f32, d, ard, kind, (n, m, batch) in itertools.product((False, True), DIMS, (False, True), ("rbf", "matern32"), SHAPES):
        dtype = torch.float32 if f32 else torch.float64
        dev, rnd, X, xnew, cparams, desc = setup(dtype, n, m, d, ard, kind, batch, 1000 * d + 10 * ard + (kind == "rbf") + n)
        stream, op = _lib.stream_ptr(dev), C.byref(desc)
        tag = f"{'f32' if f32 else 'f64'}/d{d}/{'ard' if ard else 'scalar'}/{kind}/n{n}m{m}b{batch}"

        def keep(name, tensors):
            torch.cuda.synchronize()
            for k, v in tensors.items():
                out[f"{tag}/{name}/{k}"] = v.cpu().numpy()

        blocks = ((0, 0),) + (((ROW0, NROWS),) if n == 300 else ())
        for row0, nrows in blocks:
            desc.row0, desc.nrows = row0, nrows
            rows, blk = nrows or n, f"rows{row0}+{nrows}" if nrows else "whole"
            for p in (1, 2, 3) + (() if f32 else (8,)):
                x, y = rnd(p, n), torch.empty(p, rows, device=dev, dtype=dtype)
                ws = _lib.workspace(desc, n, 1, p, dev)
                _lib.check(lib.mfx_op_apply(op, _lib.ptr(x), n, _lib.ptr(y), rows, p, 0, _lib.ptr(ws), ws.numel(), stream))
                keep(f"matvec[valu]/{blk}/p{p}", {"y": y})
            if grad_path(f32, d, n, batch) == "mfma":
                continue
            L, R = rnd(batch, rows), rnd(batch, n)
            o, st = new_grads(cparams, n, m, d, True, False, noise=True)
            ws = _lib.workspace(desc, n, 1, batch, dev)
            _lib.check(lib.mfx_op_vjp_params(op, _lib.ptr(L), rows, _lib.ptr(R), n, batch, C.byref(st), _lib.ptr(ws), ws.numel(), stream))
            keep(f"param_vjp[valu]/{blk}", {k: o[k] for k in ("ls", "s", "noise")})
        desc.row0, desc.nrows = 0, 0
        L, R = rnd(batch, n), rnd(batch, n)
        o, st = new_grads(cparams, n, m, d, False, True)
        ws = _lib.workspace(desc, n, 1, batch, dev)
        _lib.check(lib.mfx_op_vjp_params(op, _lib.ptr(L), n, _lib.ptr(R), n, batch, C.byref(st), _lib.ptr(ws), ws.numel(), stream))
        keep("input_vjp[valu]", {"X": o["X"]})

        for p in (1, 3):
            v, u = rnd(p, n), rnd(p, m)
            y, yt = torch.empty(p, m, device=dev, dtype=dtype), torch.empty(p, n, device=dev, dtype=dtype)
            ws = _lib.scratch(int(lib.mfx_gram_cross_workspace_bytes(op, m)), dev)
            _lib.check(lib.mfx_gram_cross_apply(op, _lib.ptr(xnew), m, _lib.ptr(v), n, _lib.ptr(y), m, p, _lib.ptr(ws), ws.numel(), stream))
            _lib.check(lib.mfx_gram_cross_apply_t(op, _lib.ptr(xnew), m, _lib.ptr(u), m, _lib.ptr(yt), n, p, _lib.ptr(ws), ws.numel(), stream))
            keep(f"cross_matvec[valu]/p{p}", {"y": y, "yt": yt})

        L, R, S = rnd(batch, m), rnd(batch, n), rnd(m, n + 1)
        for name, (theta, gxn, gx) in {"theta": (1, 0, 0), "xnew": (0, 1, 0), "X": (0, 0, 1), "all": (1, 1, 1)}.items():
            o, st = new_grads(cparams, n, m, d, theta, gx)
            ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_workspace_bytes(op, m, batch)), dev)
            _lib.check(lib.mfx_gram_cross_vjp(op, _lib.ptr(xnew), m, _lib.ptr(L), m, _lib.ptr(R), n, batch, C.byref(st),
                                              _lib.ptr(o["xnew"]) if gxn else None, _lib.ptr(ws), ws.numel(), stream))
            asked = [k for k, on in (("ls", theta), ("s", theta), ("xnew", gxn), ("X", gx)) if on]  # (the rest stays zero)
            keep(f"cross_vjp_factored[valu]/{name}", {k: o[k] for k in asked})
            for lds in (n, n + 1):
                Sl = S[:, :lds].contiguous()
                o, st = new_grads(cparams, n, m, d, theta, gx)
                ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_dense_workspace_bytes(op, m)), dev)
                _lib.check(lib.mfx_gram_cross_vjp_dense(op, _lib.ptr(xnew), m, _lib.ptr(Sl), lds, C.byref(st),
                                                        _lib.ptr(o["xnew"]) if gxn else None, _lib.ptr(ws), ws.numel(), stream))
                keep(f"cross_vjp_dense{'16B' if lds == n else ''}[valu]/{name}", {k: o[k] for k in asked})

        for name, xb, mb in (("sym", None, m), ("rect", X, n)):
            blk = torch.empty(m, mb, device=dev, dtype=dtype)
            ws = _lib.scratch(int(lib.mfx_gram_block_workspace_bytes(op, m, mb)), dev)
            _lib.check(lib.mfx_gram_block(op, _lib.ptr(xnew), m, _lib.ptr(xb), mb, _lib.ptr(blk), mb, _lib.ptr(ws), ws.numel(), stream))
            keep(f"gram_block[valu]/{name}", {"K": blk})
    np.savez(path, **out)


def child_time(path, reps):
    import torch
    from matfree_extensions import _lib

    lib, out = _lib.get(), {}
    n, m, batch = 8192, 1024, 16
    for f32, d in itertools.product((False, True), (8, 40)):
        dtype = torch.float32 if f32 else torch.float64
        dev, rnd, X, xnew, cparams, desc = setup(dtype, n, m, d, True, "rbf", batch, d)
        stream, op = _lib.stream_ptr(dev), C.byref(desc)
        L, R, Lm = rnd(batch, n), rnd(batch, n), rnd(batch, m)
        ws = _lib.workspace(desc, n, 1, batch, dev)
        wsx = torch.empty(int(lib.mfx_gram_cross_vjp_workspace_bytes(op, m, batch)) + 256, dtype=torch.uint8, device=dev)
        o_theta, st_theta = new_grads(cparams, n, m, d, True, False, noise=True)  # (the o_* own the memory the structs point to)
        o_x, st_x = new_grads(cparams, n, m, d, False, True)
        o_all, st_all = new_grads(cparams, n, m, d, True, True)

        def vjp(st):
            return lambda: _lib.check(lib.mfx_op_vjp_params(op, _lib.ptr(L), n, _lib.ptr(R), n, batch, C.byref(st), _lib.ptr(ws),
                                                            ws.numel(), stream))

        def cross():
            _lib.check(lib.mfx_gram_cross_vjp(op, _lib.ptr(xnew), m, _lib.ptr(Lm), m, _lib.ptr(R), n, batch, C.byref(st_all),
                                              _lib.ptr(o_all["xnew"]), _lib.ptr(wsx), wsx.numel(), stream))

        calls = {"input_vjp": vjp(st_x), "cross_vjp_factored": cross}
        if not f32:
            calls["param_vjp"] = vjp(st_theta)
        for name, fn in calls.items():
            fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            out[f"{'f32' if f32 else 'f64'}/d{d}/{name}"] = statistics.median(ms)
    json.dump(out, open(path, "w"))


def child(lib, mode, out, reps):
    env = dict(os.environ, MFX_LIBRARY_PATH=os.path.abspath(lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--out", out, "--reps", str(reps)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--child")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.path.join(ROOT, "experiments-lanczos-adjoints_amd"))
        child_bits(a.out) if a.child == "bits" else child_time(a.out, a.reps)
        print("child ok")
        return 0
    ref, cand = a.libs
    with tempfile.TemporaryDirectory() as tmp:
        if not a.time:
            child(ref, "bits", os.path.join(tmp, "ref.npz"), a.reps)
            child(cand, "bits", os.path.join(tmp, "cand.npz"), a.reps)
            x, y = dict(np.load(os.path.join(tmp, "ref.npz"))), dict(np.load(os.path.join(tmp, "cand.npz")))
            assert sorted(x) == sorted(y)
            bad = [k for k in x if not np.array_equal(x[k], y[k])]
            nonzero = sum(bool(np.any(v != 0)) and bool(np.all(np.isfinite(v))) for v in x.values())
            groups = {}
            for k in x:
                key = "/".join(k.split("/")[:1] + k.split("/")[5:6])
                groups.setdefault(key, [0, 0])
                groups[key][0] += 1
                groups[key][1] += k in bad
            for key in sorted(groups):
                print(f"{key:40s} arrays {groups[key][0]:5d}  differing {groups[key][1]}")
            for k in bad:
                print("differs:", k, float(np.abs(x[k].astype(np.float64) - y[k].astype(np.float64)).max()))
            print(f"{len(x) - len(bad)} of {len(x)} arrays bit-identical ({nonzero} finite and non-zero): reference {ref}, candidate {cand}")
            return 1 if bad else 0
        runs = []
        for i, lib in enumerate((ref, cand, ref, cand)):
            path = os.path.join(tmp, f"t{i}.json")
            child(lib, "time", path, a.reps)
            runs.append(json.load(open(path)))
        slower = 0
        print(f"median of {a.reps} repeats per run, ms (device events); margin = |reference run 1 - reference run 2|")
        print(f"{'case':34s} {'ref 1':>9s} {'cand 1':>9s} {'ref 2':>9s} {'cand 2':>9s} {'ref':>9s} {'cand':>9s} {'margin':>8s}  verdict")
        for k in runs[0]:
            r1, c1, r2, c2 = (run[k] for run in runs)
            r, c, margin = (r1 + r2) / 2, (c1 + c2) / 2, abs(r1 - r2)
            over = c - r > margin
            slower += over
            print(f"{k:34s} {r1:9.4f} {c1:9.4f} {r2:9.4f} {c2:9.4f} {r:9.4f} {c:9.4f} {margin:8.4f}  "
                  f"{'SLOWER by %.4f' % (c - r) if over else 'within' if c >= r else 'faster'}")
        print(f"{slower} of {len(runs[0])} cases slower than the reference by more than its own run-to-run difference")
        return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
