#!/usr/bin/env python3
"""Component covariance on the matrix cores: for M components of synthetic samples resident in HBM
(5 levels, n_l halving per level, about 3 GiB of samples at every M),

  ms_var / ms_mean   HIP-event time per estimate (mask pass + matrix-core launch + reduction of every chunk,
                     mlmc_accum_kernel_time) with variances / mean only (MLMC_MODE_MEAN_ONLY)
  tflops, frac       executed MFMA flops (mlmc_accum_kernel_flops) per second, and their fraction of the fp64 matrix peak
  wall_ms            host wall time of one estimate (mlmc_accum_estimate: reset + pushes + finalize)

at M = 16, 64, 256, 1024; at M = 16 also the per-pair route it replaces (M (M + 1) / 2 estimates of q_i * q_j over a
DeviceMemory storage) against estimate_mean(component_covariance(q)) on the same storage; and a 1-core NumPy einsum of the
level sums on a small n.  Prints one JSON line.
Usage: python tools/component_cov.py [--reps K] [--quick]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mlmc_amd import _lib
from mlmc_amd.engine import ComponentCovAccumulator

FP64_MFMA_PEAK_TFLOPS = 78.6
L = 5


def level_chunks(M, total_bytes, seed=0):
    """[(level, fine [M, n], coarse [M, n] | None)] as torch CUDA tensors; n_l halves per level."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    weights = [2.0 ** -l * (1 if l == 0 else 2) for l in range(L)]          # level 0 stores one value per sample
    n0 = int(total_bytes / (8 * M * sum(weights)))
    out = []
    for l in range(L):
        n = max(n0 >> l, 1)
        f = torch.randn((M, n), generator=g, device="cuda", dtype=torch.float64)
        c = None if l == 0 else f + 0.1 * torch.randn((M, n), generator=g, device="cuda", dtype=torch.float64)
        out.append((l, f, c))
    torch.cuda.synchronize()
    return out


def time_estimates(M, chunks, mean_only, reps):
    acc = ComponentCovAccumulator(M, L, mean_only=mean_only)
    acc.set_shift(np.full(M, 0.5))
    acc.estimate(chunks)                                  # warm-up (scratch allocation)
    acc.kernel_time()
    acc.kernel_flops()
    t0 = time.perf_counter()
    for _ in range(reps):
        acc.estimate(chunks)
    wall = (time.perf_counter() - t0) * 1e3 / reps
    ms, launches, _ = acc.kernel_time()
    flops = acc.kernel_flops()
    acc.close()
    return ms / reps, wall, flops / reps, launches // reps


def pair_route(M, n_per_level, reps):
    """M = 16: the reference-style route (one derived quantity per pair) against one component-covariance estimate."""
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import DeviceMemory
    spec = [QuantitySpec(name="q", unit="m", shape=(M, 1), times=[1], locations=['0'])]
    st = DeviceMemory()
    st.save_global_data(result_format=spec, level_parameters=[[0.1 ** (l + 1)] for l in range(L)])
    for l, f, c in level_chunks(M, 8.0 * M * 2 * n_per_level * 2, seed=3):
        st.set_level_samples(l, torch.stack([f, f if c is None else c], dim=-1))
    torch.cuda.synchronize()
    q = make_root_quantity(st, spec)['q']
    comps = [q[1]['0'][i, 0] for i in range(M)]
    pairs = [comps[i] * comps[j] for i in range(M) for j in range(i, M)]
    node = qe.component_covariance(q)
    qe.estimate_mean(node)
    for p in pairs[:4]:
        qe.estimate_mean(p)
    t0 = time.perf_counter()
    for _ in range(reps):
        qe.estimate_mean(node)
    xcov_ms = (time.perf_counter() - t0) * 1e3 / reps
    t0 = time.perf_counter()
    for p in pairs:
        qe.estimate_mean(p)
    pair_ms = (time.perf_counter() - t0) * 1e3
    qe.device_cache_clear()
    return dict(M=M, pairs=len(pairs), samples=int(sum(st.get_n_collected())), pair_route_ms=round(pair_ms, 2),
                component_cov_ms=round(xcov_ms, 3), speedup=round(pair_ms / xcov_ms, 1))


def numpy_baseline(M=64, n=4000):
    rng = np.random.default_rng(1)
    f = rng.normal(size=(M, n))
    c = f + 0.1 * rng.normal(size=(M, n))
    t0 = time.perf_counter()
    Y = np.einsum("ik,jk->kij", f, f, optimize=False) - np.einsum("ik,jk->kij", c, c, optimize=False)   # no BLAS: one core
    s, sp = Y.sum(axis=0), (Y * Y).sum(axis=0)
    dt = time.perf_counter() - t0
    del s, sp
    return dict(M=M, n=n, ms=round(dt * 1e3, 2), ns_per_pair_sample=round(dt * 1e9 / (n * M * M), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="0.25 GiB of samples per M")
    args = ap.parse_args()
    _lib.init(0, _lib.FLAG_TIMING)
    total = (0.25 if args.quick else 3.0) * 2 ** 30
    rows = []
    for M in (16, 64, 256, 1024):
        chunks = level_chunks(M, total, seed=M)
        ms_var, wall_var, fl_var, launches = time_estimates(M, chunks, False, args.reps)
        ms_mean, wall_mean, fl_mean, _ = time_estimates(M, chunks, True, args.reps)
        tf = fl_var / (ms_var * 1e-3) / 1e12
        rows.append(dict(M=M, n=[int(c[1].shape[1]) for c in chunks], launches=launches,
                         ms_var=round(ms_var, 3), wall_ms_var=round(wall_var, 3), ms_mean=round(ms_mean, 3),
                         wall_ms_mean=round(wall_mean, 3), mfma_flops_var=int(fl_var), tflops_var=round(tf, 2),
                         frac_var=round(tf / FP64_MFMA_PEAK_TFLOPS, 3),
                         tflops_mean=round(fl_mean / (ms_mean * 1e-3) / 1e12, 2),
                         frac_mean=round(fl_mean / (ms_mean * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS, 3)))
        del chunks
        torch.cuda.empty_cache()
    out = dict(tool="component_cov", device=_lib.device_info()["name"], peak_tflops=FP64_MFMA_PEAK_TFLOPS, levels=L, rows=rows,
               pair_route=pair_route(16, 20000 if args.quick else 200000, args.reps), numpy_1core=numpy_baseline())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
