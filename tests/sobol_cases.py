"""The scrambled Sobol' points of MLMC_SAMPLE_SOBOL (include/mlmc_hip.h) restated in plain NumPy, shared by
tests/test_sobol_cpu.py and tests/test_gpu_sobol_samples.py.  Nothing here touches the device.

Raw point i of a dimension with direction numbers V[t]: the XOR of V[t] over the set bits t of the Gray code i ^ (i >> 1).  The
scramble (keyed by `seed`, Philox of tests/sample_cases.py on the counter (c0, c1, 0, "SOBL")): digit r sits at bit 51 - r, bit
51 - r of the scrambled value is the parity of mask_r & raw with mask_r = random bits on the more significant digits and a one on
the diagonal; then a digital shift.  It is linear, so it is applied to the direction numbers.  u = (2 m + 1) 2^-53."""
import numpy as np
from scipy import special

from tests import sample_cases as sc

BITS = 52
DIMS = 1024
TAG = 0x534F424C                                       # "SOBL"
ALL = (1 << BITS) - 1


def gray(idx):
    i = np.asarray(idx, dtype=np.uint64)
    return i ^ (i >> np.uint64(1))


def raw_points(dirs, idx):
    """dirs [..., 52] uint64, idx [n]: the XOR of dirs[..., t] over the set bits t of gray(idx); returns [..., n] uint64"""
    dirs = np.asarray(dirs, dtype=np.uint64)
    g = gray(idx)
    out = np.zeros(dirs.shape[:-1] + g.shape, dtype=np.uint64)
    for t in range(BITS):
        bit = ((g >> np.uint64(t)) & np.uint64(1)).astype(bool)
        out ^= np.where(bit, dirs[..., t, None], np.uint64(0))
    return out


def word52(seed, c0, c1):
    r = sc.philox4x32_10((np.uint64(c0), np.uint64(c1), np.uint64(0), np.uint64(TAG)), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    return (int(r[0]) << 20) | (int(r[1]) >> 12)


def scramble_masks(seed, dim):
    return [(word52(seed, dim, r) & ~((1 << (BITS - r)) - 1) & ALL) | (1 << (BITS - 1 - r)) for r in range(BITS)]


def scrambled_table(seed, dims, raw_dirs):
    """raw_dirs [len(dims), 52]: the raw direction numbers of the dimensions `dims`.  Returns (dirs [len(dims), 52], shift
    [len(dims)]) as uint64: V'[t] = S_d(V[t]) and word52(d, 52)"""
    dirs = np.zeros((len(dims), BITS), dtype=np.uint64)
    shift = np.zeros(len(dims), dtype=np.uint64)
    for k, d in enumerate(dims):
        masks = scramble_masks(seed, int(d))
        for t in range(BITS):
            v = int(raw_dirs[k][t])
            dirs[k, t] = sum((bin(masks[r] & v).count("1") & 1) << (BITS - 1 - r) for r in range(BITS))
        shift[k] = word52(seed, int(d), BITS)
    return dirs, shift


_RAW = {}


def joe_kuo_numbers():
    """(poly [1024], minit [1024][13]) as lists of int: the committed data of mlmc_amd/csrc/sobol_table.hpp"""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlmc_amd", "csrc", "sobol_table.hpp")
    text = re.sub(r"//[^\n]*", "", open(path).read())
    poly = re.search(r"SOBOL_POLY\[SOBOL_DIMS\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    minit = re.search(r"SOBOL_MINIT\[SOBOL_DIMS\]\[SOBOL_MAX_DEGREE\]\s*=\s*\{(.*)\};", text, flags=re.S).group(1)
    poly = [int(v) for v in re.findall(r"\d+", poly)]
    minit = [[int(v) for v in re.findall(r"\d+", row)] for row in re.findall(r"\{([^{}]*)\}", minit)]
    assert len(poly) == len(minit) == DIMS
    return poly, minit


def raw_directions(dims):
    """raw Joe-Kuo direction numbers [len(dims), 52] by the recurrence of include/mlmc_hip.h in Python integers, from the committed
    polynomials and initial values; tests/test_sobol_cpu.py pins their points to SciPy's"""
    if "all" not in _RAW:
        poly, minit = joe_kuo_numbers()
        V = np.zeros((DIMS, BITS), dtype=np.uint64)
        for d in range(DIMS):
            p = poly[d]
            s = p.bit_length() - 1
            m = [1] * BITS if d == 0 else list(minit[d][:s])
            for k in range(len(m), BITS):
                v = m[k - s] ^ (m[k - s] << s)
                for i in range(1, s):
                    if (p >> (s - i)) & 1:
                        v ^= m[k - i] << i
                m.append(v)
            V[d] = [m[t] << (BITS - 1 - t) for t in range(BITS)]
        _RAW["all"] = V
    return _RAW["all"][np.asarray(dims, dtype=np.int64)]


def points(seed, dims, first, n):
    """m(d, i) [len(dims), n] uint64 of the points first .. first + n - 1"""
    dirs, shift = scrambled_table(seed, dims, raw_directions(dims))
    idx = np.uint64(first) + np.arange(n, dtype=np.uint64)
    return raw_points(dirs, idx) ^ shift[:, None]


def to_unit(m):
    return (np.uint64(2) * m + np.uint64(1)).astype(np.float64) * 2.0 ** -53          # below 2^53: the conversion is exact


def uniforms(seed, dim, first, n):
    """u of coordinate `dim` of the points first .. first + n - 1"""
    return to_unit(points(seed, [dim], first, n)[0])


def latent_uniforms(seed, dims, first, n):
    """[K, n]: the uniform behind latent normal k"""
    return to_unit(points(seed, list(dims), first, n))


def normals(seed, dims, first, n):
    return special.ndtri(latent_uniforms(seed, dims, first, n))
