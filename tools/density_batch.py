#!/usr/bin/env python3
"""Batched max-entropy densities against their loop: for M components x R moments x n samples per
level of synthetic per-component samples resident in HBM (DeviceMemory, 3 levels, component m shifted and scaled),

  chain_ms      Estimate.construct_densities of the M-component quantity (tol 1e-8, orth_moments_tol 1e-4)
  loop_ms       the loop of Estimate(q_m, storage, fn).construct_density over the components
  orth_ms       host orthogonalisation (construct_ortogonal_moments) of all M components, part of both
  solve_ms      the batched solve of the chain's M problems (one mlmc_maxent_solve_batch)
  single_ms     the same M problems by M mlmc_maxent_solve calls

and the solver's time per problem at B = 1, 256 and 1000 copies of one R = 25 problem.  Prints one JSON line.
Usage: python tools/density_batch.py [--quick | --config M,R,n] [--reps K]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mlmc_amd import _lib, Legendre
from mlmc_amd.estimator import Estimate, scalar_component
from mlmc_amd.quantity.quantity import make_root_quantity
from mlmc_amd.quantity.quantity_spec import QuantitySpec
from mlmc_amd.quantity import quantity_estimate as qe
from mlmc_amd.sample_storage import DeviceMemory
from mlmc_amd.tool import simple_distribution as sd

STEPS = [0.5, 0.07, 0.01]
DOM = (-3.5, 3.5)


def storage(M, n):
    g = torch.Generator(device="cuda")
    g.manual_seed(M * 7919 + n)
    shift = torch.linspace(-0.3, 0.3, M, dtype=torch.float64, device="cuda")[:, None]
    scale = torch.linspace(0.8, 1.2, M, dtype=torch.float64, device="cuda")[:, None]
    st = DeviceMemory()
    spec = [QuantitySpec(name="q", unit="m", shape=(M, 1), times=[1], locations=['0'])]
    st.save_global_data(result_format=spec, level_parameters=[[s] for s in STEPS])
    for l, h in enumerate(STEPS):
        x = torch.randn((M, n), dtype=torch.float64, device="cuda", generator=g)
        root = torch.sqrt(1e-4 + x.abs())
        fine = shift + scale * (x + h * root)
        coarse = shift + scale * (x + STEPS[l - 1] * root) if l else torch.zeros_like(fine)
        st.set_level_samples(l, torch.stack([fine, coarse], dim=-1))
    torch.cuda.synchronize()
    q = make_root_quantity(st, spec)['q'][1]['0']
    return st, q


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def run_config(M, R, n, reps):
    st, q = storage(M, n)
    fn = Legendre(R, DOM)
    comps = [scalar_component(q, m) for m in range(M)]
    est = Estimate(q, st, fn)
    chain_ms, got = timed(lambda: est.construct_densities(tol=1e-8, orth_moments_tol=1e-4), reps)
    loop_ms, _ = timed(lambda: [Estimate(c, st, fn).construct_density(tol=1e-8, orth_moments_tol=1e-4) for c in comps], reps)
    covs = qe.component_means(comps, [fn] * M, cov=True)
    orth_ms, _ = timed(lambda: [sd.construct_ortogonal_moments(fn, c, tol=1e-4) for c in covs], reps)
    distrs = [d for d, _, _, _ in got]
    args = ([d.moments_fn for d in distrs], [d.moment_means for d in distrs], [d._moment_errs for d in distrs],
            [d.domain for d in distrs])
    lam0 = [np.eye(d.approx_size)[0] * -np.log(1.0 / (d.domain[1] - d.domain[0])) for d in distrs]
    solve_ms, _ = timed(lambda: sd._solve_batch_on_device(*args, lam0, 1e-8, 100), reps)
    single_ms, _ = timed(lambda: [sd._solve_on_device(f, mu, e, dm, l0, 1e-8, 100) for f, mu, e, dm, l0 in zip(*args, lam0)], reps)
    ok = all(r.success for _, _, r, _ in got)
    del st, q
    torch.cuda.empty_cache()
    return dict(M=M, R=R, n=n, chain_ms=round(chain_ms, 3), loop_ms=round(loop_ms, 3), speedup=round(loop_ms / chain_ms, 2),
                orth_ms=round(orth_ms, 3), solve_ms=round(solve_ms, 3), single_ms=round(single_ms, 3),
                solve_speedup=round(single_ms / solve_ms, 2), r1=sorted({d.approx_size for d in distrs}), all_success=ok)


def per_problem(reps):
    from scipy import stats
    fn = Legendre(25, DOM)
    mom = sd.compute_semiexact_moments(fn, lambda x: 0.6 * stats.norm(-0.5, 0.8).pdf(x) + 0.4 * stats.norm(1.0, 0.6).pdf(x))
    lam0 = np.eye(25)[0] * -np.log(1.0 / (DOM[1] - DOM[0]))
    out = {}
    for B in (1, 256, 1000):
        ms, res = timed(lambda: sd._solve_batch_on_device([fn] * B, [mom] * B, [np.ones(25)] * B, [DOM] * B, [lam0] * B, 1e-8, 100), reps)
        out[str(B)] = dict(total_ms=round(ms, 3), us_per_problem=round(ms * 1e3 / B, 2), nit=int(res[0][3].nit))
    single_ms, _ = timed(lambda: sd._solve_on_device(fn, mom, np.ones(25), DOM, lam0, 1e-8, 100), reps)
    out["single_solve_ms"] = round(single_ms, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="M in {1, 8}, R = 25, 10^4 samples only")
    ap.add_argument("--config", help="one configuration M,R,n (e.g. 64,25,10000), for a profiler run")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    _lib.init(0)
    Ms, Rs, ns = ((1, 8), (25,), (10_000,)) if a.quick else ((1, 8, 64, 256), (13, 25, 49), (10_000, 1_000_000))
    if a.config:
        M, R, n = (int(v) for v in a.config.split(","))
        Ms, Rs, ns = (M,), (R,), (n,)
    rows = [run_config(M, R, n, a.reps) for n in ns for R in Rs for M in Ms]
    print(json.dumps(dict(tool="density_batch", device=_lib.device_info()["name"], configs=rows, solver=per_problem(a.reps))))


if __name__ == "__main__":
    main()
