#!/usr/bin/env python3
"""Batched bootstrap against the loop: a scalar quantity resident in HBM (a DeviceMemory storage, 5
levels of n samples, one stored chunk per level), Legendre moments of size R, B replicates, half of every level requested:

  loop_ms      host wall time of Estimate.est_bootstrap(B, sample_vector)  (B estimates of a gathered sub-sample)
  batch_ms     host wall time of Estimate.est_bootstrap_batch(B, sample_vector, seed)
  contract_ms  HIP-event time of the contraction launches (keep bytes, k_bs_contract, k_bs_reduce) of one accumulation of the
               same chunks and sizes (engine.BootstrapAccumulator), mfma_frac = executed MFMA flops / contract time / 78.6 TFLOP/s
  rng_ms       HIP-event time of the weight passes (tile counts, expansion); rng_share = rng_ms / (rng_ms + contract_ms)

at n = 10^4 .. 10^7 and R = 16, 64, B = 100, 300.  Prints one JSON line per point and a summary line.
Usage: python tools/bootstrap_batch.py [--quick]   (MLMC_HIP_TIMING is switched on here: the event times need it)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["MLMC_HIP_TIMING"] = "1"
import numpy as np
import torch

from mlmc_amd import _lib, engine

L = 5
PEAK = 78.6e12


def storage(n, seed=0):
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import DeviceMemory
    g = torch.Generator(device="cuda").manual_seed(seed)
    spec = [QuantitySpec(name="q", unit="m", shape=(1, 1), times=[1], locations=['0'])]
    st = DeviceMemory()
    st.save_global_data(result_format=spec, level_parameters=[[0.1 ** (l + 1)] for l in range(L)])
    for l in range(L):
        f = torch.randn((1, n), generator=g, device="cuda", dtype=torch.float64)
        c = f + 0.1 * 0.5 ** l * torch.randn((1, n), generator=g, device="cuda", dtype=torch.float64)
        st.set_level_samples(l, torch.stack([f, c], dim=-1))
    torch.cuda.synchronize()
    return st, make_root_quantity(st, spec)['q'][1]['0'][0, 0]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_times(q, st, fn, B, k, seed):
    """One accumulation of the storage's chunks with the sizes est_bootstrap_batch draws: (contract ms, rng ms, MFMA flops)."""
    from mlmc_amd.quantity import quantity_estimate as qe
    acc = engine.BootstrapAccumulator(fn, 1, L, B)
    acc.kernel_time()
    N = st.get_n_collected()
    for cs in st.chunks():
        l = int(cs.level_id)
        fine, coarse = qe._chunk_for_device(q, qe.lowering.plan_for(q), cs, qe._level_stamps(q.get_quantity_storage()), True)
        fine = fine.reshape(1, -1).contiguous()
        coarse = None if coarse is None else coarse.reshape(1, -1).contiguous()
        sizes = qe.bootstrap_sizes(seed, l, 0, k[l], N[l], fine.shape[1], B)
        acc.accum(l, fine, coarse, sizes, seed, qe.bootstrap_stream(l, 0))
    acc.finalize()
    out = acc.kernel_time()
    acc.close()
    return out


def point(n, R, B):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st, q = storage(n, seed=n + R)
    fn = Legendre(R, (-4.0, 4.0))
    k = [n // 2] * L
    est = Estimate(q, st, fn)
    est.est_bootstrap_batch(2, sample_vector=k, seed=1)              # warm-up: lowering, cache, first allocations
    est.est_bootstrap(2, sample_vector=k)
    batch_ms = wall(lambda: est.est_bootstrap_batch(B, sample_vector=k, seed=7))
    loop_ms = wall(lambda: est.est_bootstrap(B, sample_vector=k))
    c_ms, r_ms, flops = kernel_times(q, st, fn, B, k, 7)
    return dict(n=n, R=R, B=B, L=L, loop_ms=round(loop_ms, 2), batch_ms=round(batch_ms, 2), speedup=round(loop_ms / batch_ms, 1),
                contract_ms=round(c_ms, 3), mfma_tflops=round(flops / (c_ms * 1e-3) / 1e12, 2) if c_ms > 0 else None,
                mfma_frac=round(flops / (c_ms * 1e-3) / PEAK, 3) if c_ms > 0 else None, rng_ms=round(r_ms, 3),
                rng_share=round(r_ms / (r_ms + c_ms), 3) if r_ms + c_ms > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="n = 10^4, 10^5 only")
    args = ap.parse_args()
    _lib.init(0, _lib.FLAG_TIMING)
    ns = [10 ** 4, 10 ** 5] if args.quick else [10 ** 4, 10 ** 5, 10 ** 6, 10 ** 7]
    rows = []
    for n in ns:
        for R in (16, 64):
            for B in (100, 300):
                r = point(n, R, B)
                rows.append(r)
                print(json.dumps(r), flush=True)
    print(json.dumps(dict(tool="bootstrap_batch", device=_lib.device_info()["name"], points=len(rows),
                          min_speedup=min(r["speedup"] for r in rows), max_speedup=max(r["speedup"] for r in rows))))


if __name__ == "__main__":
    main()
