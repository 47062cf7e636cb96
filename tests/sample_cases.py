"""The uniforms of the sampling entry (include/mlmc_hip.h, mlmc_density_sample_batch) restated in plain NumPy, shared by
tests/test_density_samples_cpu.py and tests/test_gpu_density_samples.py.  Nothing here touches the device.

Uniform k of stream s under `seed`: Philox4x32-10 keyed by (low word of seed, high word of seed) on the counter
(i_lo, i_hi, s, 0x53414D50), i = k >> 1, gives r0 .. r3; (hi, lo) = (r0, r1) for even k and (r2, r3) for odd k;
m = (hi << 20) | (lo >> 12); u = (2 m + 1) 2^-53.  Draw j uses uniform j, or with the antithetic flag uniform j >> 1 and, for odd
j, 1 - u."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
TAG = 0x53414D50
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

# the DKW bound at confidence 1 - 1e-9 for n = 16384: sqrt(ln(2 / 1e-9) / (2 n))
DKW_N = 16384
DKW_BOUND = float(np.sqrt(np.log(2 / 1e-9) / (2 * DKW_N)))


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars; returns four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def stream_uniforms(seed, stream, index):
    """uniform `index` (uint64 array) of the stream"""
    k = np.asarray(index, dtype=np.uint64)
    i = k >> np.uint64(1)
    r = philox4x32_10((i & MASK, i >> S32, np.uint64(stream), np.uint64(TAG)), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    odd = (k & np.uint64(1)).astype(bool)
    hi = np.where(odd, r[2], r[0]).astype(np.uint64)
    lo = np.where(odd, r[3], r[1]).astype(np.uint64)
    m = (hi << np.uint64(20)) | (lo >> np.uint64(12))
    return (np.uint64(2) * m + np.uint64(1)).astype(np.float64) * 2.0 ** -53          # below 2^53: the conversion is exact


def uniforms(seed, stream, first, n, antithetic=False):
    """u_j of the draws j = first .. first + n - 1"""
    j = np.uint64(first) + np.arange(n, dtype=np.uint64)
    if not antithetic:
        return stream_uniforms(seed, stream, j)
    u = stream_uniforms(seed, stream, j >> np.uint64(1))
    return np.where((j & np.uint64(1)).astype(bool), 1.0 - u, u)


def kolmogorov_distance(f):
    """sup-distance between the empirical distribution function of a sample and the CDF whose values at the sample are `f`"""
    f = np.sort(np.asarray(f, dtype=np.longdouble))
    n = f.size
    k = np.arange(1, n + 1, dtype=np.longdouble)
    return float(max(np.max(k / n - f), np.max(f - (k - 1) / n)))
