#!/usr/bin/env python3
"""Per-component bootstrap against the loop of scalar calls: a vector quantity of M components resident
in HBM (a DeviceMemory storage, 5 levels of n samples, one stored chunk per level), Legendre moments of size R with a domain of
its own per component, B replicates, half of every level requested:

  loop_ms      host wall time of the M calls Estimate(scalar_component(q, m), st, fns[m]).est_bootstrap_batch(B, k, seed)
  comp_ms      host wall time of Estimate(q, st).est_bootstrap_components(B, k, fns, seed)
               (both: median of the repetitions, the two alternating on the same device; `reps` says how many were taken)
  contract_ms  HIP-event time of the contraction launches (keep bytes, k_bs_contract and k_bs_reduce under the per-component layout) of one
               accumulation of the same chunks and sizes (engine.ComponentBootstrapAccumulator), mfma_frac = executed MFMA flops /
               contract time / 78.6 TFLOP/s
  rng_ms       HIP-event time of the weight passes (tile counts, expansion)

at M = 16, 64, 256, R = 16, 25, B = 300 and n = 10^4, 10^5, 10^6.  With --bands: Estimate.bootstrap_component_quantiles at M = 64,
R = 25, B = 300 (19 200 max-entropy problems), split into the bootstrap pass, the batched solve and the batched quantiles, and the
share of successful solves.  Prints one JSON line per point and a summary line.
Usage: python tools/bootstrap_components.py [--quick] [--bands]   (MLMC_HIP_TIMING is switched on here: the event times need it)"""
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
PEAK = 78.6e12


def storage(n, M, seed=0):
    from mlmc_amd.quantity.quantity import make_root_quantity
    from mlmc_amd.quantity.quantity_spec import QuantitySpec
    from mlmc_amd.sample_storage import DeviceMemory
    g = torch.Generator(device="cuda").manual_seed(seed)
    spec = [QuantitySpec(name="q", unit="m", shape=(M, 1), times=[1], locations=['0'])]
    st = DeviceMemory()
    st.save_global_data(result_format=spec, level_parameters=[[0.1 ** (l + 1)] for l in range(L)])
    shift = 0.01 * torch.arange(M, device="cuda", dtype=torch.float64)[:, None]
    for l in range(L):
        f = torch.randn((M, n), generator=g, device="cuda", dtype=torch.float64) + shift
        c = f + 0.1 * 0.5 ** l * torch.randn((M, n), generator=g, device="cuda", dtype=torch.float64)
        st.set_level_samples(l, torch.stack([f, c], dim=-1))
    torch.cuda.synchronize()
    q = make_root_quantity(st, spec)['q'][1]['0']
    return st, (q[0, 0] if M == 1 else q)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_times(q, st, fns, R, B, k, seed):
    """One accumulation of the storage's chunks with the sizes the call draws: (contract ms, rng ms, MFMA flops)."""
    from mlmc_amd.quantity import quantity_estimate as qe
    M = len(fns)
    acc = engine.ComponentBootstrapAccumulator(fns, R, L, B)
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


def point(n, M, R, B, max_reps=3, budget_s=20.0):
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate, scalar_component
    st, q = storage(n, M, seed=n + M + R)
    fns = [Legendre(R, (-5.0 - 0.01 * m, 5.0 + 0.02 * m)) for m in range(M)]
    k = [n // 2] * L
    est = Estimate(q, st, fns[0])
    scalars = [Estimate(scalar_component(q, m), st, fns[m]) for m in range(M)]

    def comp(b=B):
        return est.est_bootstrap_components(b, sample_vector=k, moments_fns=fns, seed=7)

    def loop(b=B):
        return [e.est_bootstrap_batch(b, sample_vector=k, seed=7) for e in scalars]
    comp(2)                                                   # warm-up: lowering, cache, first allocations, code objects
    loop(2)
    comp_ms, loop_ms = [], []
    t0 = time.perf_counter()
    while len(comp_ms) < max_reps and (not comp_ms or time.perf_counter() - t0 < budget_s):
        comp_ms.append(wall(comp))
        loop_ms.append(wall(loop))
    # the same replicates from both routes (checked on the last repetition's inputs, outside the timed windows)
    a, ref = comp(), scalars[M - 1].est_bootstrap_batch(B, sample_vector=k, seed=7)
    assert np.array_equal(a.n_samples[:, :, M - 1], ref.n_samples)
    assert np.allclose(a.l_means[:, :, M - 1], ref.l_means, rtol=1e-10, atol=1e-13)
    c_ms, r_ms, flops = kernel_times(q, st, fns, R, B, k, 7)
    cm, lm = statistics.median(comp_ms), statistics.median(loop_ms)
    return dict(n=n, M=M, R=R, B=B, L=L, reps=len(comp_ms), loop_ms=round(lm, 2), comp_ms=round(cm, 2), speedup=round(lm / cm, 2),
                comp_all_ms=[round(v, 2) for v in comp_ms], loop_all_ms=[round(v, 2) for v in loop_ms],
                contract_ms=round(c_ms, 3), mfma_tflops=round(flops / (c_ms * 1e-3) / 1e12, 2) if c_ms > 0 else None,
                mfma_frac=round(flops / (c_ms * 1e-3) / PEAK, 3) if c_ms > 0 else None, rng_ms=round(r_ms, 3))


def bands(n, M=64, R=25, B=300):
    """bootstrap_component_quantiles and its three parts, each timed on its own (the same inputs)"""
    from mlmc_amd import Legendre
    from mlmc_amd.estimator import Estimate
    from mlmc_amd.quantity import quantity_estimate as qe
    from mlmc_amd.tool import simple_distribution as sd
    st, q = storage(n, M, seed=n + M + R)
    fns = [Legendre(R, tuple(d)) for d in Estimate.estimate_domains(q, st)]
    k = [n // 2] * L
    probs = np.array([0.05, 0.5, 0.95])
    est = Estimate(q, st, fns[0])
    dens = est.construct_densities(moments_fns=fns)
    est.bootstrap_component_quantiles(probs, 2, sample_vector=k, seed=7, moments_fns=fns, densities=dens)        # warm-up
    t0 = time.perf_counter()
    res = est.bootstrap_component_quantiles(probs, B, sample_vector=k, seed=7, moments_fns=fns, densities=dens)
    total_ms = (time.perf_counter() - t0) * 1e3
    out = {}
    pass_ms = wall(lambda: out.update(p=qe.bootstrap_component_moments(q, fns, B, np.array(k), 7)))
    nb, s, _ = out["p"]
    t0 = time.perf_counter()
    distrs = []
    for b in range(B):
        for m in range(M):
            mobj = dens[m][3]
            mu = np.sum([(s[b, l, m] / float(nb[b, l, m])) @ mobj._base_matrix.T for l in range(L)], axis=0)
            distrs.append(sd.SimpleDistribution(mobj, np.stack((mu, np.ones(mobj.size)), axis=1), domain=mobj.domain))
    host_ms = (time.perf_counter() - t0) * 1e3
    solve_ms = wall(lambda: out.update(r=sd.estimate_densities_minimize(distrs, 1e-8, 0.0)))
    quant_ms = wall(lambda: sd.quantiles(distrs, probs))
    ok = np.array([bool(r.success) for r in out["r"]]).reshape(B, M)
    assert np.array_equal(ok, res.success)
    return dict(bands=True, n=n, M=M, R=R, B=B, L=L, problems=B * M, orth_sizes=sorted({int(d[3].size) for d in dens}),
                total_ms=round(total_ms, 1), pass_ms=round(pass_ms, 1), host_build_ms=round(host_ms, 1), solve_ms=round(solve_ms, 1),
                solve_ms_per_1000=round(solve_ms / (B * M) * 1000, 2), quantiles_ms=round(quant_ms, 1),
                full_sample_ok=int(sum(bool(d[2].success) for d in dens)), ok_share=round(float(ok.mean()), 4),
                ok_share_min_component=round(float(ok.mean(axis=0).min()), 4),
                band_width_median=float(np.nanmedian(res.hi - res.lo)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="n = 10^4, 10^5 and M = 16, 64 only")
    ap.add_argument("--bands", action="store_true", help="the quantile bands at M = 64, R = 25, B = 300 instead of the grid")
    args = ap.parse_args()
    _lib.init(0, _lib.FLAG_TIMING)
    if args.bands:
        for n in (10 ** 4, 10 ** 5):
            print(json.dumps(bands(n)), flush=True)
        return
    ns = [10 ** 4, 10 ** 5] if args.quick else [10 ** 4, 10 ** 5, 10 ** 6]
    Ms = [16, 64] if args.quick else [16, 64, 256]
    rows = []
    for n in ns:
        for M in Ms:
            for R in (16, 25):
                r = point(n, M, R, 300)
                rows.append(r)
                print(json.dumps(r), flush=True)
    print(json.dumps(dict(tool="bootstrap_components", device=_lib.device_info()["name"], points=len(rows),
                          min_speedup=min(r["speedup"] for r in rows), max_speedup=max(r["speedup"] for r in rows))))


if __name__ == "__main__":
    main()
