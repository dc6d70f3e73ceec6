"""Work-precision study of the anisotropic wave equation: the Krylov depth of `expm_arnoldi` against the step count of fixed-step
Runge-Kutta baselines, value and parameter gradient of <u, y(1)> measured against dopri8 with 50 steps in fp64.

The reference's experiment of the same name on this build's kernels: the vector field is the matrix-free stencil operator
(`pde_wave_anisotropic(...).flat`), every solver a native driver (`pde_util.solver_expm` / `pde_util.solver_rk`).  Same command line
and the same four arrays per method (`wp_<method>_Ns`, `_ts`, `_errors_fwd`, `_errors_rev` under `results/`).  Without the data set on
disk (`./data/pde_wave/<res>x<res>_data_{inputs,targets,parameter}.npy`) a synthetic one of the same shapes is generated.
`diffrax:tsit5+recursive_checkpoint` is accepted and refused with the reason (`rk_tableaux`): its coefficients are not available.

  python workprecision.py --resolution 32 --method diffrax:dopri5+backsolve [--num_steps_max 10] [--num_runs 1]

`--adaptive` (off by default; nothing else changes without it) replaces the sweep over step counts of a `diffrax:` method by a sweep
over tolerances: `pde_util.solver_rk_adaptive` on the method's embedded pair (dopri5, heun) at rtol = 10^-1 .. 10^-(num_steps_max - 1),
atol = 1e-3 rtol, the arrays saved as `wp_<method>+adaptive_*`.
"""

import argparse
import os
import sys
import time

import numpy as np
import torch

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "../../.."))
sys.path.insert(0, os.path.join(_ROOT, "experiments-lanczos-adjoints_amd"))

from matfree_extensions.util import exp_util, pde_util  # noqa: E402

METHODS = {
    "diffrax:euler+backsolve": ("euler", "backsolve"),
    "diffrax:heun+recursive_checkpoint": ("heun", "recursive_checkpoint"),
    "diffrax:tsit5+recursive_checkpoint": ("tsit5", "recursive_checkpoint"),
    "diffrax:dopri5+backsolve": ("dopri5", "backsolve"),
}


def load_data(res, device):
    path = f"./data/pde_wave/{res}x{res}"
    if os.path.exists(f"{path}_data_parameter.npy"):
        y0 = np.load(f"{path}_data_inputs.npy")[0]
        parameter = np.load(f"{path}_data_parameter.npy")
    else:
        rng = np.random.default_rng(res)
        xs = np.linspace(0.0, 1.0, res)
        bump = np.exp(-40.0 * ((xs[:, None] - 0.5) ** 2 + (xs[None, :] - 0.4) ** 2))
        y0 = np.stack([bump, np.zeros_like(bump)])
        parameter = 0.3 + 0.1 * rng.standard_normal((res, res))
        print(f"(synthetic stand-in for the {res} x {res} wave data set)")
    return torch.tensor(y0, dtype=torch.float64, device=device), torch.tensor(parameter, dtype=torch.float64, device=device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, required=True)
    ap.add_argument("--method", type=str, required=True)
    ap.add_argument("--num_runs", type=int, default=1)
    ap.add_argument("--num_steps_max", type=int, default=10)
    ap.add_argument("--adaptive", action="store_true", help="sweep tolerances of the adaptive-step solver instead of step counts")
    args = ap.parse_args()
    if args.adaptive and args.method == "arnoldi":
        raise ValueError("--adaptive sweeps the tolerance of a Runge-Kutta pair; arnoldi has no step size")
    if args.method != "arnoldi" and args.method not in METHODS:
        raise ValueError(f"The method {args.method} is not supported.")
    dev = torch.device("cuda:0")
    res = args.resolution
    y0, parameter = load_data(res, dev)
    dx = 1.0 / (res - 1)
    rhs_of, _ = pde_util.pde_wave_anisotropic(parameter, pde_util.stencil_laplacian(dx), constrain=torch.square,
                                              boundary=pde_util.boundary_neumann())
    u = torch.rand(y0.shape, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1421))

    def value_and_grad(make_solver):
        def run():
            p = parameter.clone().requires_grad_(True)
            y1, info = make_solver(rhs_of(scale=p).flat)(y0)
            value = (u * y1).sum()
            (grad,) = torch.autograd.grad(value, p)
            return value.detach(), grad, info

        return run

    def timed(run):
        ts = []
        for _ in range(args.num_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return ts

    truth = value_and_grad(lambda field: pde_util.solver_rk(0.0, 1.0, field, num_steps=50, method="dopri8", adjoint="direct"))
    value, gradient, _ = truth()
    error = pde_util.loss_mse_relative(nugget=torch.finfo(torch.float64).eps)
    Ns, ts_all, errors_fwd, errors_rev = [], [], [], []
    for nstp in range(1, args.num_steps_max):
        if nstp > parameter.numel():
            print("The Krylov depth would exceed the matrix size.")
            break
        if args.adaptive:
            method, adjoint = METHODS[args.method]
            make = lambda field: pde_util.solver_rk_adaptive(0.0, 1.0, field, method=method, rtol=10.0**-nstp, atol=10.0 ** -(nstp + 3),  # noqa: E731
                                                             adjoint=adjoint, max_steps=100000 if adjoint == "backsolve" else 4096)
        elif args.method == "arnoldi":
            make = lambda field: pde_util.solver_expm(0.0, 1.0, field, expm=pde_util.expm_arnoldi(nstp))  # noqa: E731
        else:
            method, adjoint = METHODS[args.method]
            make = lambda field: pde_util.solver_rk(0.0, 1.0, field, num_steps=nstp, method=method, adjoint=adjoint)  # noqa: E731
        run = value_and_grad(make)
        f, df, info = run()
        fwd = float(torch.sqrt(error(f, targets=value)))
        rev = float(torch.sqrt(error(df, targets=gradient)))
        Ns.append(int(info["num_matvecs"]))
        errors_fwd.append(fwd)
        errors_rev.append(rev)
        ts_all.append(timed(run))
        print(f"N={Ns[-1]}, fwd={fwd:.1e}, rev={rev:.1e}, t={min(ts_all[-1]):.2e} s", flush=True)
    directory = exp_util.matching_directory(__file__, "results/")
    os.makedirs(directory, exist_ok=True)
    if args.adaptive:
        args.method += "+adaptive"
    np.save(f"{directory}/wp_{args.method}_Ns", np.asarray(Ns))
    np.save(f"{directory}/wp_{args.method}_ts", np.asarray(ts_all))
    np.save(f"{directory}/wp_{args.method}_errors_fwd", np.asarray(errors_fwd))
    np.save(f"{directory}/wp_{args.method}_errors_rev", np.asarray(errors_rev))


if __name__ == "__main__":
    main()
