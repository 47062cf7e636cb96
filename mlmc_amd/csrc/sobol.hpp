// The scrambled Sobol' points of MLMC_SAMPLE_SOBOL (include/mlmc_hip.h): what the sampling entries (density.hip) and the normals
// kernel (sobol.hip) share.  The host builds, once per call, one row of SOBOL_ROW words per distinct dimension of the call: the 52
// scrambled direction numbers V'[t] and the digital shift.  The device only XORs.
#pragma once
#include "common.hpp"

namespace mlmc {

constexpr int SOBOL_BITS = 52;
constexpr int SOBOL_ROW = SOBOL_BITS + 1;              // V'[0 .. 51] | shift
constexpr int64_t SOBOL_MAX_INDEX = (int64_t)1 << SOBOL_BITS;

// m of point idx (< 2^52) from its dimension's row: shift ^ XOR of V'[t] over the set bits t of the Gray code of idx.  The Gray code
// is below 2^52, so t <= 51.  The Gray codes of idx - 1 and idx differ in bit ctz(idx): m(idx) = m(idx - 1) ^ V'[ctz(idx)].
__device__ __forceinline__ uint64_t sobol_point(const uint64_t *row, uint64_t idx) {
    uint64_t g = idx ^ (idx >> 1), m = row[SOBOL_BITS];
    while (g) {
        m ^= row[__builtin_ctzll(g)];
        g &= g - 1;
    }
    return m;
}
// u = (2 m + 1) 2^-53: exact, 0 < u < 1, and 1 - u is exact
__device__ __forceinline__ double sobol_unit(uint64_t m) { return (double)(int64_t)(2 * m + 1) * 0x1p-53; }

// raw Joe-Kuo direction numbers V[t] = m_{t+1} << (51 - t) of dimension d < SOBOL_DIMS (host)
void sobol_directions(uint32_t d, uint64_t *V);
// row [SOBOL_ROW] of dimension d under `seed`: the scrambled direction numbers and the shift (host)
void sobol_scrambled_row(uint64_t seed, uint32_t d, uint64_t *row);
// The table of a call: dims[i] (NULL: i), i < n, are checked (< SOBOL_DIMS, else an error that names `what` i), their distinct
// values get one row each in `table`, in the order of first appearance, and slot[i] is the row of dims[i].
int sobol_call_table(const char *fn, const char *what, uint64_t seed, const uint32_t *dims, int n, std::vector<uint64_t> &table,
                     std::vector<uint32_t> &slot);

// Z[k * ldz + c] = normcdfinv(coordinate of point first + c in the dimension of row slots[k] of `table`), c < ncols
// (k_cop_sobol_normals); slots [K] and table: device
void cop_launch_sobol_normals(hipStream_t st, const uint64_t *table, const uint32_t *slots, int K, int64_t first, int64_t ncols,
                              double *Z, int64_t ldz);

}  // namespace mlmc
