#!/usr/bin/env python3
"""Per-component domains in one batched selection: for M components of synthetic samples resident in
HBM (a DeviceMemory storage, 5 levels, n samples per level),

  loop_ms      host wall time of the loop [Estimate.estimate_domain(scalar_component(q, m), st) for m in range(M)]
  batch_ms     host wall time of Estimate.estimate_domains(q, st) (one tree evaluation and one mlmc_percentiles_rows call per
               level; equal to the loop bit for bit, checked)
  select_ms    host wall time of one engine.row_percentiles call on a resident [M, n] tensor (the selection alone)

at M = 16, 64, 256, 1024 and n = 10^4, 10^5; and engine.row_percentiles against engine.percentiles on one row of 10^7 values
in HBM, with the effective read bandwidth (8 n bytes per call).  Prints one JSON line.
Usage: python tools/domain_batch.py [--reps K] [--quick]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mlmc_amd import _lib, engine

L = 5


def storage(M, n, seed=0):
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import DeviceMemory
    g = torch.Generator(device="cuda").manual_seed(seed)
    spec = [QuantitySpec(name="q", unit="m", shape=(M, 1), times=[1], locations=['0'])]
    st = DeviceMemory()
    st.save_global_data(result_format=spec, level_parameters=[[0.1 ** (l + 1)] for l in range(L)])
    shift = torch.linspace(-3.0, 3.0, M, device="cuda", dtype=torch.float64)[:, None]
    for l in range(L):
        f = torch.randn((M, n), generator=g, device="cuda", dtype=torch.float64) + shift
        c = f + 0.1 * torch.randn((M, n), generator=g, device="cuda", dtype=torch.float64)
        st.set_level_samples(l, torch.stack([f, c], dim=-1))
    torch.cuda.synchronize()
    return st, make_root_quantity(st, spec)['q']


def wall(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, r


def domains_row(M, n, reps):
    from mlmc_amd.estimator import Estimate, scalar_component
    from mlmc_amd.quantity import quantity_estimate as qe
    st, q = storage(M, n, seed=M + n)
    comps = [scalar_component(q, m) for m in range(M)]
    Estimate.estimate_domains(q, st)                                 # warm-up (scratch, lowering caches)
    for c in comps[:2]:
        Estimate.estimate_domain(c, st)
    batch_ms, got = wall(lambda: Estimate.estimate_domains(q, st), reps)
    loop_ms, want = wall(lambda: np.array([Estimate.estimate_domain(c, st) for c in comps]), 1)
    x = torch.randn((M, n), device="cuda", dtype=torch.float64)
    engine.row_percentiles(x, [1.0, 99.0])
    select_ms, _ = wall(lambda: engine.row_percentiles(x, [1.0, 99.0]), reps)
    qe.device_cache_clear()
    return dict(M=M, n=n, levels=L, loop_ms=round(loop_ms, 2), batch_ms=round(batch_ms, 3), speedup=round(loop_ms / batch_ms, 1),
                select_ms=round(select_ms, 3), bit_identical=bool(np.array_equal(got, want)))


def long_row(n, reps):
    x = torch.randn((1, n), device="cuda", dtype=torch.float64)
    qs = [1.0, 99.0]
    engine.row_percentiles(x, qs)
    engine.percentiles(x[0], qs)
    rows_ms, a = wall(lambda: engine.row_percentiles(x, qs), reps)
    scalar_ms, b = wall(lambda: engine.percentiles(x[0], qs), reps)
    return dict(M=1, n=n, row_percentiles_ms=round(rows_ms, 3), percentiles_ms=round(scalar_ms, 3),
                row_percentiles_gbps=round(8 * n / (rows_ms * 1e-3) / 1e9, 1), percentiles_gbps=round(8 * n / (scalar_ms * 1e-3) / 1e9, 1),
                bit_identical=bool(np.array_equal(a[0], b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="M = 16 and 64 only, n = 10^4")
    args = ap.parse_args()
    _lib.init(0)
    rows = []
    for n in ((10_000,) if args.quick else (10_000, 100_000)):
        for M in ((16, 64) if args.quick else (16, 64, 256, 1024)):
            rows.append(domains_row(M, n, args.reps))
            torch.cuda.empty_cache()
    out = dict(tool="domain_batch", device=_lib.device_info()["name"], rows=rows, long_row=long_row(10_000_000, args.reps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
