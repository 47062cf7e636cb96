#!/usr/bin/env python3
"""Per-component moment estimates against their loop: for M components x R Legendre moments x n
samples per level of synthetic per-component samples resident in HBM (DeviceMemory, 4 levels, component m shifted and scaled),

  batched_ms    Estimate.estimate_component_diff_vars_regression of the M-component quantity (one device pass per chunk)
  loop_ms       the loop of Estimate(q_m, storage, fn).estimate_diff_vars_regression over the components
  entry_ms      one mlmc_accum_estimate_multi_var call on the gathered chunks (launches + one wait: an upper bound of the
                kernel time; rocprofv3 --kernel-trace gives the kernels alone)
  mean_only_ms  with --mean-only: one mlmc_accum_estimate_multi call (no squares) on the same chunks, K = linearize.extended_size
                of the moments (2 R - 1 for Legendre), the pass behind Estimate.construct_densities; mean_only_K names K
  evals_per_s   moment evaluations (fine and coarse values x R) per second of entry_ms
  fp64_frac     flops by the count of DESIGN 3.1 (14 R per pair, 8 R at level 0) per entry_ms against 78.6 TFLOP/s

Prints one JSON line.  Usage: python tools/component_moments.py [--quick | --config M,R,n] [--reps K] [--no-loop] [--mean-only]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mlmc_amd import _lib, Legendre, linearize
from mlmc_amd.estimator import Estimate, scalar_component
from mlmc_amd.quantity.quantity import make_root_quantity
from mlmc_amd.quantity.quantity_spec import QuantitySpec
from mlmc_amd.quantity import quantity_estimate as qe
from mlmc_amd.sample_storage import DeviceMemory

STEPS = [0.5, 0.15, 0.05, 0.01]
FP64_PEAK = 78.6e12


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
        del x, root, fine, coarse
    st.save_n_ops([(l, (float(1.0 / h), n)) for l, h in enumerate(STEPS)])
    torch.cuda.synchronize()
    q = make_root_quantity(st, spec)['q'][1]['0']
    return st, q


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def entry_call(q, fns, mean_only=False):
    """The C entry alone on the quantity's gathered chunks (what component_level_sums times beyond the gathering); mean_only:
    mlmc_accum_estimate_multi on the extended members of the moments instead."""
    if mean_only:
        fns = [fn.change_size(linearize.extended_size(fn)) for fn in fns]
    M, R = len(fns), fns[0].size
    n_levels, keep, args = qe._component_chunks(q, M, "component_moments")
    n = np.zeros((n_levels, M), dtype=np.int64)
    n_rm = np.zeros_like(n)
    outs = [np.zeros((n_levels, M, R)) for _ in range(1 if mean_only else 2)]
    handles = qe._basis_handles(fns)
    entry = getattr(_lib.lib(), "mlmc_accum_estimate_multi" if mean_only else "mlmc_accum_estimate_multi_var")

    def call():
        _lib.check(entry(M, handles, R, n_levels, *args, _lib.ptr(n), _lib.ptr(n_rm), *[_lib.ptr(o) for o in outs]))
        return keep, fns
    return call


def run_config(M, R, n, reps, loop, mean_only=False):
    st, q = storage(M, n)
    fns = [Legendre(R, (-3.5 + 0.3 * m / max(M - 1, 1), 3.5 + 0.3 * m / max(M - 1, 1))) for m in range(M)]
    est = Estimate(q, st, fns[0])
    n_created = [n] * len(STEPS)
    batched_ms, (reg, _) = timed(lambda: est.estimate_component_diff_vars_regression(n_created, moments_fns=fns), reps)
    loop_ms = None
    if loop:
        comps = [scalar_component(q, m) for m in range(M)]
        loop_ms, _ = timed(lambda: [Estimate(c, st, f).estimate_diff_vars_regression(n_created) for c, f in zip(comps, fns)],
                           max(1, reps // 2))
    entry_ms, _ = timed(entry_call(q, fns), reps)
    mean = {}
    if mean_only:
        mean_ms, _ = timed(entry_call(q, fns, mean_only=True), reps)
        mean = dict(mean_only_ms=round(mean_ms, 4), mean_only_K=linearize.extended_size(fns[0]))
    L = len(STEPS)
    evals = M * n * R * (1 + 2 * (L - 1))                         # fine values at level 0, fine and coarse above
    flops = M * n * R * (8 + 14 * (L - 1))
    row = dict(M=M, R=R, n=n, L=L, batched_ms=round(batched_ms, 3), loop_ms=None if loop_ms is None else round(loop_ms, 3),
               speedup=None if loop_ms is None else round(loop_ms / batched_ms, 2), entry_ms=round(entry_ms, 4),
               evals_per_s=float("%.4g" % (evals / (entry_ms * 1e-3))),
               fp64_frac=round(flops / (entry_ms * 1e-3) / FP64_PEAK, 3), finite=bool(np.all(np.isfinite(reg))), **mean)
    del st, q, est
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="M in {1, 8}, R = 25, 10^4 samples only")
    ap.add_argument("--config", help="one configuration M,R,n (e.g. 64,32,1000000), for a profiler run")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true", help="do not time the per-component loop")
    ap.add_argument("--mean-only", action="store_true", help="also time mlmc_accum_estimate_multi (mean-only, K = 2 R - 1)")
    a = ap.parse_args()
    _lib.init(0)
    Ms, Rs, ns = ((1, 8), (25,), (10_000,)) if a.quick else ((1, 8, 64, 256), (13, 25, 64), (10_000, 1_000_000))
    if a.config:
        M, R, n = (int(v) for v in a.config.split(","))
        Ms, Rs, ns = (M,), (R,), (n,)
    rows = []
    for n in ns:
        for R in Rs:
            for M in Ms:
                rows.append(run_config(M, R, n, a.reps, not a.no_loop, a.mean_only))
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)       # progress
    print(json.dumps(dict(tool="component_moments", device=_lib.device_info()["name"], rows=rows)))


if __name__ == "__main__":
    main()
