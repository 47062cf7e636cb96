#!/usr/bin/env python3
"""Level diagnostics of every component at size: for M components x n samples per level of synthetic
per-component samples resident in HBM (DeviceMemory, 4 levels, component m shifted and scaled),

  wall_ms       Estimate.estimate_level_diagnostics of the M-component quantity (chunks resident after the first call)
  event_ms      HIP events around one mlmc_level_diagnostics call on the gathered chunks (its launches, the download of the
                per-chunk results and the gaps between them; rocprofv3 --kernel-trace gives the kernels alone)
  alg_bytes     bytes the algorithm moves: 16 per pair and 8 at level 0, times its two passes
  tb_per_s      alg_bytes / event_ms
  scalar_*      the same for the moments kernel of DESIGN 3.1 with R = 8 Legendre moments on the same chunks in the same process
                (mlmc_accum_estimate of a LevelAccumulator with M components, one pass: the project's memory-bound yardstick)
  percomp_*     and for mlmc_accum_estimate_multi_var, the per-component moments pass (own domain per component), R = 8
  today_*       what a user has without the feature: loop_ms, the loop of estimate_mean(q_m) (mean and variance of the
                differences only), and numpy_ms, the kurtosis from NumPy on downloaded samples (None above --today-max values)

Prints one JSON line.  Usage: python tools/level_diagnostics.py [--quick | --config M,n] [--reps K] [--today-max V]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mlmc_amd import _lib, Legendre
from mlmc_amd.engine import LevelAccumulator
from mlmc_amd.estimator import Estimate, scalar_component
from mlmc_amd.quantity.quantity import make_root_quantity
from mlmc_amd.quantity.quantity_spec import QuantitySpec
from mlmc_amd.quantity import quantity_estimate as qe
from mlmc_amd.sample_storage import DeviceMemory

STEPS = [0.5, 0.15, 0.05, 0.01]


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
    st.save_n_ops([(l, (float(n / h), n)) for l, h in enumerate(STEPS)])
    torch.cuda.synchronize()
    return st, make_root_quantity(st, spec)['q'][1]['0']


def wall(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def events(call, reps):
    """Best HIP-event time of `call` (an entry of the library, which runs on torch's current stream here)."""
    call()
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def run_config(M, n, reps, today_max):
    st, q = storage(M, n)
    L = len(STEPS)
    est = Estimate(q, st)
    wall_ms, d = wall(est.estimate_level_diagnostics, reps)
    lib = _lib.lib()
    n_levels, keep, args = qe._component_chunks(q, M, "level_diagnostics")
    cnt, cnt_rm, stats = np.zeros((L, M), dtype=np.int64), np.zeros((L, M), dtype=np.int64), np.zeros((L, M, 9))
    event_ms = events(lambda: _lib.check(lib.mlmc_level_diagnostics(M, n_levels, *args, _lib.ptr(cnt), _lib.ptr(cnt_rm),
                                                                     _lib.ptr(stats))), reps)
    fns = [Legendre(8, (-6.0, 6.0)) for _ in range(M)]
    handles = qe._basis_handles(fns)
    s, sp = np.zeros((L, M, 8)), np.zeros((L, M, 8))
    moments_ms = events(lambda: _lib.check(lib.mlmc_accum_estimate_multi_var(M, handles, 8, n_levels, *args, _lib.ptr(cnt),
                                                                             _lib.ptr(cnt_rm), _lib.ptr(s), _lib.ptr(sp))), reps)
    acc = LevelAccumulator(fns[0], n_levels, n_comp=M)
    chunks = [(int(lv), f, c) for lv, (f, c) in zip(keep[-1][0], keep[:-1])]
    scalar_ms = events(lambda: acc.estimate(chunks), reps)
    acc.close()
    pass_bytes = M * n * (8 + 16 * (L - 1))
    row = dict(M=M, n=n, L=L, wall_ms=round(wall_ms, 3), event_ms=round(event_ms, 4), alg_bytes=2 * pass_bytes,
               tb_per_s=round(2 * pass_bytes / (event_ms * 1e-3) / 1e12, 3), scalar_event_ms=round(scalar_ms, 4),
               scalar_alg_bytes=pass_bytes, scalar_tb_per_s=round(pass_bytes / (scalar_ms * 1e-3) / 1e12, 3),
               percomp_event_ms=round(moments_ms, 4), percomp_tb_per_s=round(pass_bytes / (moments_ms * 1e-3) / 1e12, 3),
               today_loop_ms=None, today_numpy_ms=None, max_kurtosis=float(np.nanmax(d.kurtosis_diff)),
               finite=bool(np.all(np.isfinite(d.kurtosis_diff))))
    del keep
    if M * n <= today_max:
        comps = [scalar_component(q, m) for m in range(M)]
        row["today_loop_ms"] = round(wall(lambda: [qe.estimate_mean(c) for c in comps], max(1, reps // 2))[0], 3)

        def numpy_kurtosis():
            out = np.empty((L, M))
            for l in range(L):
                x = st._levels[l].cpu().numpy()                        # [M, n, 2]: the download is part of what it costs
                y = x[:, :, 0] - (x[:, :, 1] if l else 0.0)
                dlt = y - np.mean(y, axis=1, keepdims=True)
                out[l] = np.mean(dlt ** 4, axis=1) / np.mean(dlt ** 2, axis=1) ** 2
            return out
        row["today_numpy_ms"], k = wall(numpy_kurtosis, 1)
        row["today_numpy_ms"] = round(row["today_numpy_ms"], 3)
        row["kurtosis_agrees"] = bool(np.allclose(k, d.kurtosis_diff, rtol=1e-9))
    del st, q, est
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="M = 1 and 8 at 10^4 samples only")
    ap.add_argument("--config", help="one configuration M,n (e.g. 64,1000000), for a profiler run")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--today-max", type=float, default=1e7, help="largest M x n for the loop / NumPy comparison")
    a = ap.parse_args()
    _lib.init(0)
    _lib.use_torch_stream()                                            # the events above bracket the library's launches
    configs = [(1, 10_000), (8, 10_000)] if a.quick else [(1, 100_000), (1, 10_000_000), (64, 10_000), (64, 1_000_000)]
    if a.config:
        configs = [tuple(int(v) for v in a.config.split(","))]
    rows = []
    for M, n in configs:
        rows.append(run_config(M, n, a.reps, a.today_max))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)       # progress
    print(json.dumps(dict(tool="level_diagnostics", device=_lib.device_info()["name"], rows=rows)))


if __name__ == "__main__":
    main()
