#!/usr/bin/env python3
"""Bootstrap of the component covariance against the loop of sub-sampled estimates: a vector quantity
of M components resident in HBM (a DeviceMemory storage, 5 levels of n samples, one stored chunk per level), B = 300 replicates,
half of every level requested:

  loop_ms      host wall time of B calls estimate_mean(component_covariance(quantity.subsample(k), shift)) -- the only way to the
               replicates without the batched entry (unseeded; every call walks the storage and pays the fixed host cost)
  call_ms      host wall time of Estimate(q, st).est_bootstrap_component_covariance(B, k, seed) (it includes the estimate_mean
               pass for the shift)
               (both: median of three repetitions, the two alternating on the same device in the same session; all are printed)
  contract_ms  HIP-event time of the contraction launches (keep bytes, k_bs_xcov_contract, k_bs_xcov_reduce) of one accumulation
               of the same chunks and sizes (engine.ComponentCovBootstrapAccumulator); mfma_frac = executed MFMA flops /
               contract time / 78.6 TFLOP/s
  rng_ms       HIP-event time of the weight passes (tile counts, expansion)

at M = 12, 16, 64 and n = 10^4, 10^5 per level, followed by one bootstrap_joint_exceedance timing (M = 12, n = 10^4, B = 300,
2^12 points x 8 seeds per replicate).  Prints one JSON line per point and a summary line.
Usage: python tools/bootstrap_xcov.py [--quick]   (--quick: the grid above; without it n = 10^6 is added.  MLMC_HIP_TIMING is
switched on here: the event times need it)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["MLMC_HIP_TIMING"] = "1"
import numpy as np
import torch

from mlmc_amd import _lib, engine

L = 5
B = 300
PEAK = 78.6e12


def storage(n, M, seed=0):
    """correlated components: a common factor with a weight that grows with the component"""
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import DeviceMemory
    g = torch.Generator(device="cuda").manual_seed(seed)
    spec = [QuantitySpec(name="q", unit="m", shape=(M, 1), times=[1], locations=['0'])]
    st = DeviceMemory()
    st.save_global_data(result_format=spec, level_parameters=[[0.1 ** (l + 1)] for l in range(L)])
    shift = 0.01 * torch.arange(M, device="cuda", dtype=torch.float64)[:, None]
    load = torch.linspace(0.2, 0.8, M, device="cuda", dtype=torch.float64)[:, None]
    for l in range(L):
        common = torch.randn((1, n), generator=g, device="cuda", dtype=torch.float64)
        f = load * common + torch.sqrt(1.0 - load * load) * torch.randn((M, n), generator=g, device="cuda", dtype=torch.float64) + shift
        c = f + 0.1 * 0.5 ** l * torch.randn((M, n), generator=g, device="cuda", dtype=torch.float64)
        st.set_level_samples(l, torch.stack([f, c], dim=-1))
    torch.cuda.synchronize()
    return st, make_root_quantity(st, spec)['q'][1]['0']


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_times(q, st, M, k, seed):
    """One accumulation of the storage's chunks with the sizes the call draws: (contract ms, rng ms, MFMA flops)."""
    from mlmc_amd.quantity import quantity_estimate as qe
    acc = engine.ComponentCovBootstrapAccumulator(M, L, B)
    acc.kernel_time()
    N = st.get_n_collected()
    for cs in st.chunks():
        l = int(cs.level_id)
        fine, coarse = qe._chunk_for_device(q, qe.lowering.plan_for(q), cs, qe._level_stamps(q.get_quantity_storage()), True)
        fine = fine.reshape(M, -1).contiguous()
        coarse = None if coarse is None else coarse.reshape(M, -1).contiguous()
        sizes = qe.bootstrap_sizes(seed, l, 0, k[l], N[l], fine.shape[1], B)
        acc.accum(l, fine, coarse, sizes, seed, qe.bootstrap_stream(l, 0))
    acc.finalize()
    out = acc.kernel_time()
    acc.close()
    return out


def point(n, M, reps=3):
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    st, q = storage(n, M, seed=n + M)
    k = [n // 2] * L
    est = Estimate(q, st)
    shift = np.asarray(qe.estimate_mean(q).mean, dtype=np.float64).reshape(M)

    def call(b=B):
        return est.est_bootstrap_component_covariance(b, sample_vector=k, seed=7)

    def loop(b=B):
        return [qe.estimate_mean(qe.component_covariance(q.subsample(sample_vec=k), shift)).mean for _ in range(b)]
    call(2)                                                   # warm-up: lowering, cache, first allocations, code objects
    loop(2)
    call_ms, loop_ms = [], []
    for _ in range(reps):
        call_ms.append(wall(call))
        loop_ms.append(wall(loop))
    # both routes estimate the same thing: the spread of an off-diagonal entry over the replicates agrees within its own noise
    r = call()
    cov_loop = np.array(loop()).reshape(B, M, M)
    sd_call, sd_loop = np.std(r.cov[:, 0, M - 1], ddof=1), np.std(cov_loop[:, 0, M - 1], ddof=1)
    assert r.ok.all() and 0.7 < sd_call / sd_loop < 1.4, (sd_call, sd_loop)
    c_ms, r_ms, flops = kernel_times(q, st, M, k, 7)
    cm, lm = statistics.median(call_ms), statistics.median(loop_ms)
    return dict(n=n, M=M, B=B, L=L, columns=1 + M + M * (M + 1) // 2, loop_ms=round(lm, 2), call_ms=round(cm, 2),
                speedup=round(lm / cm, 2), call_all_ms=[round(v, 2) for v in call_ms], loop_all_ms=[round(v, 2) for v in loop_ms],
                contract_ms=round(c_ms, 3), rng_ms=round(r_ms, 3), mfma_tflops=round(flops / (c_ms * 1e-3) / 1e12, 2) if c_ms > 0 else None,
                mfma_frac=round(flops / (c_ms * 1e-3) / PEAK, 4) if c_ms > 0 else None,
                sd_ratio_call_over_loop=round(float(sd_call / sd_loop), 3))


def exceedance(n=10 ** 4, M=12):
    """one bootstrap_joint_exceedance call: all components above their 80 % quantile, marginals fixed"""
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    st, q = storage(n, M, seed=n + M)
    fns = [Legendre(9, tuple(d)) for d in Estimate.estimate_domains(q, st)]
    est = Estimate(q, st, fns[0])
    dens = est.construct_densities(moments_fns=fns)
    t = est.estimate_component_quantiles([0.8], densities=dens)[0][:, 0]
    k = [n // 2] * L
    est.bootstrap_joint_exceedance(t, 2, sample_vector=k, seed=7, densities=dens)                     # warm-up
    out = {}
    ms = wall(lambda: out.update(r=est.bootstrap_joint_exceedance(t, B, sample_vector=k, seed=7, densities=dens)))
    pass_ms = wall(lambda: est.est_bootstrap_component_covariance(B, sample_vector=k, seed=7))
    r = out["r"]
    return dict(exceedance=True, n=n, M=M, B=B, L=L, points=2 ** 12, seeds=8, total_ms=round(ms, 1), covariance_pass_ms=round(pass_ms, 1),
                ms_per_replicate_integral=round((ms - pass_ms) / (B + 1), 2), prob=float(r.prob[0]), qmc_stderr=float(r.stderr[0]),
                lo=float(r.lo[0]), hi=float(r.hi[0]), n_ok=int(r.n_ok))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="n = 10^4, 10^5 only")
    args = ap.parse_args()
    _lib.init(0, _lib.FLAG_TIMING)
    rows = []
    for n in ([10 ** 4, 10 ** 5] if args.quick else [10 ** 4, 10 ** 5, 10 ** 6]):
        for M in (12, 16, 64):
            r = point(n, M)
            rows.append(r)
            print(json.dumps(r), flush=True)
    print(json.dumps(exceedance()), flush=True)
    print(json.dumps(dict(tool="bootstrap_xcov", device=_lib.device_info()["name"], points=len(rows),
                          min_speedup=min(r["speedup"] for r in rows), max_speedup=max(r["speedup"] for r in rows))))


if __name__ == "__main__":
    main()
