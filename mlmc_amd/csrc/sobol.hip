// Scrambled Sobol' points for the sampling entries (MLMC_SAMPLE_SOBOL, include/mlmc_hip.h): the host side of the table and the
// kernel of the latent normals (gfx950).
//
//   host   : Joe-Kuo direction numbers from sobol_table.hpp by the recurrence, the linear matrix scramble and the digital shift
//            keyed by Philox (the keying of q_uniform, copula.hpp, tag word "SOBL"), mlmc_sobol_table, and the table of a call
//            (one row per distinct dimension).  The scramble is linear over GF(2), so it is applied to the 52 direction numbers
//            of a dimension once per call and a point stays an XOR of direction numbers.
//   k_cop_sobol_normals : Z[k][c] = normcdfinv(coordinate of point first + c in the dimension of row k), beside k_cop_normals
//            (copula.hip).  One thread per element, consecutive lanes write consecutive draws; the row's 53 words are staged in
//            LDS once per workgroup and a thread forms its point directly from the set bits of its Gray code (on average half
//            as many XORs as the index has bits), so the value does not depend on the grid.  As in k_cop_normals there is no
//            loop around normcdfinv.
#include <algorithm>

#include "sobol.hpp"
#include "sobol_table.hpp"

namespace mlmc {

constexpr int SOBOL_NORMAL_THREADS = 256;

void sobol_directions(uint32_t d, uint64_t *V) {
    uint64_t m[SOBOL_BITS];
    const uint32_t p = SOBOL_POLY[d];
    int s = 0;
    while ((p >> (s + 1)) != 0) ++s;                   // the degree; 0 for dimension 0
    for (int k = 0; k < SOBOL_BITS; ++k) {
        if (s == 0) m[k] = 1;
        else if (k < s) m[k] = SOBOL_MINIT[d][k];
        else {
            uint64_t v = m[k - s] ^ (m[k - s] << s);
            for (int i = 1; i < s; ++i)
                if ((p >> (s - i)) & 1) v ^= m[k - i] << i;
            m[k] = v;                                  // odd and below 2^(k + 1)
        }
    }
    for (int t = 0; t < SOBOL_BITS; ++t) V[t] = m[t] << (SOBOL_BITS - 1 - t);
}

// Philox4x32-10 on the host, keyed as q_uniform: the 52-bit word (r0 << 20) | (r1 >> 12) of the counter (c0, c1, 0, "SOBL")
static uint64_t sobol_word52(uint64_t seed, uint32_t c0, uint32_t c1) {
    uint32_t c[4] = {c0, c1, 0u, 0x534F424Cu};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return ((uint64_t)c[0] << 20) | (uint64_t)(c[1] >> 12);
}

void sobol_scrambled_row(uint64_t seed, uint32_t d, uint64_t *row) {
    constexpr uint64_t all = ((uint64_t)1 << SOBOL_BITS) - 1;
    uint64_t V[SOBOL_BITS], mask[SOBOL_BITS];
    sobol_directions(d, V);
    // digit r sits at bit 51 - r: random bits on the more significant digits, a one on the diagonal
    for (int r = 0; r < SOBOL_BITS; ++r) {
        const uint64_t low = ((uint64_t)1 << (SOBOL_BITS - r)) - 1;
        mask[r] = (sobol_word52(seed, d, (uint32_t)r) & ~low & all) | ((uint64_t)1 << (SOBOL_BITS - 1 - r));
    }
    for (int t = 0; t < SOBOL_BITS; ++t) {
        uint64_t v = 0;
        for (int r = 0; r < SOBOL_BITS; ++r) v |= (uint64_t)(__builtin_popcountll(mask[r] & V[t]) & 1) << (SOBOL_BITS - 1 - r);
        row[t] = v;
    }
    row[SOBOL_BITS] = sobol_word52(seed, d, SOBOL_BITS);
}

int sobol_call_table(const char *fn, const char *what, uint64_t seed, const uint32_t *dims, int n, std::vector<uint64_t> &table,
                     std::vector<uint32_t> &slot) {
    std::vector<int32_t> row_of(SOBOL_DIMS, -1);
    slot.resize((size_t)n);
    table.clear();
    for (int i = 0; i < n; ++i) {
        const uint32_t d = dims ? dims[i] : (uint32_t)i;
        if (d >= (uint32_t)SOBOL_DIMS)
            return fail(std::string(fn) + ": " + what + " " + std::to_string(i) + ": stream " + std::to_string(d) +
                        " is not a Sobol' dimension (MLMC_SAMPLE_SOBOL: streams are dimensions below 1024)");
        if (row_of[d] < 0) {
            row_of[d] = (int32_t)(table.size() / SOBOL_ROW);
            table.resize(table.size() + SOBOL_ROW);
            sobol_scrambled_row(seed, d, table.data() + table.size() - SOBOL_ROW);
        }
        slot[i] = (uint32_t)row_of[d];
    }
    return 0;
}

__global__ __launch_bounds__(SOBOL_NORMAL_THREADS) void k_cop_sobol_normals(const uint64_t *__restrict__ table,
                                                                            const uint32_t *__restrict__ slots, int64_t first,
                                                                            int64_t ncols, double *__restrict__ Z, int64_t ldz) {
    __shared__ uint64_t row[SOBOL_ROW];
    const int k = blockIdx.y;
    if (threadIdx.x < SOBOL_ROW) row[threadIdx.x] = table[(int64_t)slots[k] * SOBOL_ROW + threadIdx.x];
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    // an odd multiple of 2^-53 in (0, 1): z is finite
    Z[(int64_t)k * ldz + c] = normcdfinv(sobol_unit(sobol_point(row, (uint64_t)(first + c))));
}

void cop_launch_sobol_normals(hipStream_t st, const uint64_t *table, const uint32_t *slots, int K, int64_t first, int64_t ncols,
                              double *Z, int64_t ldz) {
    // one thread per element, row k of a launch = blockIdx.y: more rows than a grid has in y go in several launches
    for (int k0 = 0; k0 < K; k0 += 65535) {
        const dim3 grid((unsigned)((ncols + SOBOL_NORMAL_THREADS - 1) / SOBOL_NORMAL_THREADS), (unsigned)std::min(K - k0, 65535));
        hipLaunchKernelGGL(k_cop_sobol_normals, grid, dim3(SOBOL_NORMAL_THREADS), 0, st, table, slots + k0, first, ncols,
                           Z + (int64_t)k0 * ldz, ldz);
    }
}

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_sobol_table(uint64_t seed, int32_t scramble, const uint32_t *dims, int32_t nd, uint64_t *dirs_out, uint64_t *shift_out) {
    if (nd < 0) return fail("mlmc_sobol_table: nd < 0");
    if (nd == 0) return 0;
    if (!dims || !dirs_out || !shift_out) return fail("mlmc_sobol_table: null argument");
    if (scramble != 0 && scramble != 1) return fail("mlmc_sobol_table: scramble is 0 or 1");
    for (int i = 0; i < nd; ++i)
        if (dims[i] >= (uint32_t)SOBOL_DIMS)
            return fail("mlmc_sobol_table: dims[" + std::to_string(i) + "] = " + std::to_string(dims[i]) + " is not below 1024");
    for (int i = 0; i < nd; ++i) {
        uint64_t row[SOBOL_ROW];
        if (scramble) sobol_scrambled_row(seed, dims[i], row);
        else {
            sobol_directions(dims[i], row);
            row[SOBOL_BITS] = 0;
        }
        std::copy(row, row + SOBOL_BITS, dirs_out + (size_t)i * SOBOL_BITS);
        shift_out[i] = row[SOBOL_BITS];
    }
    return 0;
}

}  // extern "C"
