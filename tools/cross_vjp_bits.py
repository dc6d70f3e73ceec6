#!/usr/bin/env python3
"""Bitwise A/B of the gradient sweeps between two builds of libmfx.so (the sweeps use no atomics: same order of sums, same bits).

  MFX_LIBRARY_PATH=old/libmfx.so python tools/cross_vjp_bits.py --save old.pt
  MFX_LIBRARY_PATH=new/libmfx.so python tools/cross_vjp_bits.py --save new.pt
  python tools/cross_vjp_bits.py --compare old.pt new.pt        # exit status 1 and the differing cases if any bit differs

Cases: fp32 / fp64; d in {3, 12, 20, 40} (DPAD 4 and 12: one launch; DPAD 32: two; wide: selections); scalar and ARD lengthscale;
RBF and Matern-5/2; m = 70 owners (a partly dead workgroup with dead waves), n = 300 columns (three splits, a 12-column tail);
dense weights with leading dimension 300 (vector loads) and 301 (scalar loads); theta only, each owner only, and both; one test
point on a training point.  Entry points: mfx_gram_cross_vjp, mfx_gram_cross_vjp_dense, mfx_op_vjp_params (theta, and the inputs)."""
import argparse
import ctypes as C
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiments-lanczos-adjoints_amd"))
M, N, BATCH = 70, 300, 3
REQUESTS = {"theta": (1, 0, 0), "xs": (0, 1, 0), "X": (0, 0, 1), "theta+xs": (1, 1, 0), "theta+X": (1, 0, 1), "all": (1, 1, 1)}


def run():
    from matfree_extensions import _lib
    from matfree_extensions.operators import RbfGramOp

    dev = torch.device("cuda:0")
    lib, stream, out = _lib.get(), _lib.stream_ptr(dev), {}
    for dtype, d, ard, kind in itertools.product((torch.float32, torch.float64), (3, 12, 20, 40), (False, True), ("rbf", "matern52")):
        g = torch.Generator(device=dev).manual_seed(1000 * d + 10 * ard + (kind == "rbf"))
        X = torch.randn(N, d, device=dev, generator=g, dtype=dtype)
        xs = torch.randn(M, d, device=dev, generator=g, dtype=dtype)
        xs[0] = X[5]
        L = torch.randn(BATCH, M, device=dev, generator=g, dtype=dtype)
        R = torch.randn(BATCH, N, device=dev, generator=g, dtype=dtype)
        Ln = torch.randn(BATCH, N, device=dev, generator=g, dtype=dtype)
        S = torch.randn(M, N + 1, device=dev, generator=g, dtype=dtype)
        raw = (torch.linspace(-0.3, 0.4, d, device=dev, dtype=dtype) if ard else torch.tensor(0.2, device=dev, dtype=dtype),
               torch.tensor(0.1, device=dev, dtype=dtype), torch.tensor(-1.0, device=dev, dtype=dtype))
        op = RbfGramOp(X, kernel=kind)
        cparams = op.constrain(*raw)
        desc = op.descriptor(cparams, dtype, N)
        tag = f"{'f32' if dtype == torch.float32 else 'f64'}/d{d}/{'ard' if ard else 'scalar'}/{kind}"

        def grads(theta, x):
            o = {"ls": torch.zeros_like(cparams[0]), "s": torch.zeros_like(cparams[1]), "noise": torch.zeros_like(cparams[2]),
                 "X": torch.zeros(N, d, dtype=dtype, device=dev), "xs": torch.zeros(M, d, dtype=dtype, device=dev)}
            st = _lib.OpGrads()
            if theta:
                st.lengthscale, st.outputscale = o["ls"].data_ptr(), o["s"].data_ptr()
            if x:
                st.x = o["X"].data_ptr()
            return o, st

        for name, (theta, gxs, gx) in REQUESTS.items():
            o, st = grads(theta, gx)
            ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_workspace_bytes(C.byref(desc), M, BATCH)), dev)
            _lib.check(lib.mfx_gram_cross_vjp(C.byref(desc), _lib.ptr(xs), M, _lib.ptr(L), M, _lib.ptr(R), N, BATCH, C.byref(st),
                                              _lib.ptr(o["xs"]) if gxs else None, _lib.ptr(ws), ws.numel(), stream))
            torch.cuda.synchronize()
            out[f"{tag}/factored/{name}"] = {k: v.cpu() for k, v in o.items()}
            for lds in (N, N + 1):
                Sl = S[:, :lds].contiguous()
                o, st = grads(theta, gx)
                ws = _lib.scratch(int(lib.mfx_gram_cross_vjp_dense_workspace_bytes(C.byref(desc), M)), dev)
                _lib.check(lib.mfx_gram_cross_vjp_dense(C.byref(desc), _lib.ptr(xs), M, _lib.ptr(Sl), lds, C.byref(st),
                                                        _lib.ptr(o["xs"]) if gxs else None, _lib.ptr(ws), ws.numel(), stream))
                torch.cuda.synchronize()
                out[f"{tag}/dense{lds}/{name}"] = {k: v.cpu() for k, v in o.items()}
        for name, (theta, x) in {"theta": (1, 0), "X": (0, 1)}.items():  # the square sweeps
            o, st = grads(theta, x)
            if theta:
                st.noise = o["noise"].data_ptr()
            ws = _lib.workspace(desc, N, 1, BATCH, dev)
            _lib.check(lib.mfx_op_vjp_params(C.byref(desc), _lib.ptr(Ln), N, _lib.ptr(R), N, BATCH, C.byref(st), _lib.ptr(ws), ws.numel(),
                                             stream))
            torch.cuda.synchronize()
            out[f"{tag}/square/{name}"] = {k: v.cpu() for k, v in o.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.save:
        out = run()
        torch.save(out, args.save)
        print(f"saved {len(out)} cases to {args.save}")
        return 0
    a, b = (torch.load(p) for p in args.compare)
    assert a.keys() == b.keys()
    bad = [(case, k) for case in a for k in a[case] if not torch.equal(a[case][k], b[case][k])]
    nonzero = sum(bool(v.abs().max() > 0) for case in a for v in a[case].values())
    for case, k in bad:
        print("differs:", case, k, float((a[case][k].double() - b[case][k].double()).abs().max()))
    print(f"{len(a)} cases, {nonzero} non-zero outputs, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
