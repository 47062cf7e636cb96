// Batched, seeded bootstrap of the moment estimates (Estimate.est_bootstrap_batch), gfx950.
//
// Replicate b of a stored chunk of n samples picks s_b of them uniformly with replacement (RNG.choice(chunk, s_b, axis=1)), i.e.
// integer weights w_b ~ Multinomial(s_b, uniform over n).  Its level sums are sum_i w_bi [keep_i, d_i, d_i o d_i], d_i the row of
// moment differences of sample i (fine - coarse, all M components x R moments), keep_i the mask of the moments kernels.  The
// moments are evaluated once per stored sample and replicate group; the B-fold work is the contraction W [B x n] . Phi [n x 2 M R]
// on the fp64 matrix cores (v_mfma_f64_16x16x4_f64: replicates on the M axis, samples on K, columns on N).
//
// Weights without a global scatter: a multinomial over n positions equals a multinomial over tiles of BS_TILE positions (the
// tile numbers of s_b uniform positions) followed by uniform positions inside each tile.
//   pass A (k_bs_tile_counts): s_b positions pos = hi64(r64 * n), two per Philox call; only pos / BS_TILE is kept, counted in an
//     LDS histogram (segments of BS_SEG_TILES tiles) and added to counts[b][t] with integer atomics -- exact, order-free.
//   pass B (k_bs_expand): one workgroup per (tile, replicate) draws counts[b][t] positions hi32(r32 * tile size) inside the tile,
//     four per Philox call, into an LDS histogram, and writes the tile's weights.
// Philox4x32-10 is keyed by the 64-bit seed; the counter is (draw index, replicate, tile | ~0 for pass A, stream), where the stream
// names the (level, chunk) -- never the batch size, the grid or a position in a group.  mlmc_bootstrap_weights writes the weights
// of a replicate range; mlmc_bootstrap_accum runs the same two kernels into a bounded scratch slab and contracts it, so both see
// the same weights bit for bit.
//
// Accumulation of one chunk: replicates in groups of BG (multiples of 64), samples in ranges of nr (whole tiles, a function of n
// and the column count only); per (group, range): keep bytes (k_bs_keep), the weight slab [BG][nr] (pass B), the contraction
// (k_bs_contract: grid (512-sample slice, 64-replicate tile, 16 JT-column block), partial rows per workgroup) and a fixed-order
// reduction into the level totals (k_bs_reduce).  A replicate's sums therefore do not depend on B, and runs are bit-identical.
// Scratch (tile counts, slab, partials, keep bytes) stays below 64 MiB; the totals [L][B][2 M R] are the size of the result.
//
// Per-component route (mlmc_bootstrap_create_multi, Estimate.est_bootstrap_components): one basis and one mask per component, the
// same weights, the same plan, the same k_bs_contract and k_bs_reduce under another column layout (BsPerComponent instead of
// BsSharedBasis below), keep bytes from k_bs_keep_multi, components in groups of at most 2048 columns.
//
// Component covariance of the replicates (mlmc_bootstrap_create_xcov, Estimate.est_bootstrap_component_covariance): no basis; the
// columns are the keep flag, the M shifted first moments f~_m - c~_m and the M (M + 1) / 2 upper-triangle products
// f~_i f~_j - c~_i c~_j (f~ = f - a, c~ = c - a).  The same weights, plan, replicate groups and sample ranges; a contraction of its
// own (k_bs_xcov_contract: all 256 threads fill Phi, one MFMA per 16-column tile and k-step) and its fixed-order reduction
// (k_bs_xcov_reduce), columns in groups of at most 2048.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "device_basis.hpp"

namespace mlmc {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int BS_TILE = 4096;              // positions per tile (pass A / pass B)
constexpr int BS_SEG_TILES = 8192;         // tiles per LDS histogram of pass A (32 KiB)
constexpr int BS_REPS = 64;                // replicates per contraction workgroup: 4 waves x 16 MFMA rows
constexpr int BS_KB = 64;                  // samples per batch of the contraction
constexpr int BS_SW = 512;                 // samples per contraction workgroup
constexpr int BS_TPR_MAX = 8;              // tiles per sample range (nr <= 32768)
constexpr int BS_NY_MAX = 4;               // 64-replicate tiles per group (BG <= 256)
constexpr int64_t BS_MAX_N = (int64_t)61440 * BS_TILE;   // samples per chunk: tile counts of 64 replicates within 15 MiB
constexpr int BS_MAX_COLS = 2048;          // M * R
constexpr size_t BS_COUNTS_BYTES = (size_t)15 << 20;
constexpr size_t BS_W_BYTES = (size_t)BS_NY_MAX * BS_REPS * BS_TPR_MAX * BS_TILE * 4;     // 32 MiB
constexpr size_t BS_PART_BYTES = (size_t)16 << 20;

__device__ __forceinline__ void bs_philox(uint32_t (&c)[4], uint64_t seed) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// pass A.  grid (workgroups per replicate, replicates, tile segments); sizes[b] picks of replicate b0 + b.
__global__ __launch_bounds__(256) void k_bs_tile_counts(int64_t n, int64_t n_tiles, const int64_t *__restrict__ sizes, int64_t b0,
                                                        int64_t pairs_per_wg, uint64_t seed, uint32_t stream,
                                                        int32_t *__restrict__ counts) {
    __shared__ int hist[BS_SEG_TILES];
    const int64_t s = sizes[blockIdx.y];
    const int64_t n_pairs = (s + 1) / 2;
    const int64_t p0 = (int64_t)blockIdx.x * pairs_per_wg;
    if (p0 >= n_pairs) return;                                   // (uniform over the workgroup)
    const int64_t seg0 = (int64_t)blockIdx.z * BS_SEG_TILES;
    const int nseg = (int)std::min((int64_t)BS_SEG_TILES, n_tiles - seg0);
    for (int t = threadIdx.x; t < nseg; t += blockDim.x) hist[t] = 0;
    __syncthreads();
    const int64_t p1 = std::min(n_pairs, p0 + pairs_per_wg);
    const uint32_t b = (uint32_t)(b0 + blockIdx.y);
    for (int64_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
        uint32_t c[4] = {(uint32_t)p, b, 0xFFFFFFFFu, stream};
        bs_philox(c, seed);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (2 * p + h >= s) break;
            const uint64_t r = ((uint64_t)c[2 * h + 1] << 32) | c[2 * h];
            const int64_t t = (int64_t)(__umul64hi(r, (uint64_t)n) / BS_TILE) - seg0;
            if (t >= 0 && t < nseg) atomicAdd(&hist[t], 1);
        }
    }
    __syncthreads();
    int32_t *__restrict__ row = counts + (int64_t)blockIdx.y * n_tiles + seg0;
    for (int t = threadIdx.x; t < nseg; t += blockDim.x)
        if (hist[t]) atomicAdd(&row[t], hist[t]);
}

// pass B.  grid (tiles t_first .. t_first + gridDim.x - 1, replicates); w[b][t * BS_TILE - col0 + i] = weight of sample i of tile t.
__global__ __launch_bounds__(256) void k_bs_expand(int64_t n, int64_t n_tiles, int64_t t_first, const int32_t *__restrict__ counts,
                                                   int64_t b0, uint64_t seed, uint32_t stream, int32_t *__restrict__ w, int64_t ldw,
                                                   int64_t col0) {
    __shared__ int hist[BS_TILE];
    const int64_t t = t_first + blockIdx.x;
    const int m = counts[(int64_t)blockIdx.y * n_tiles + t];
    const int64_t first = t * BS_TILE;
    const uint32_t size = (uint32_t)std::min((int64_t)BS_TILE, n - first);
    for (int i = threadIdx.x; i < BS_TILE; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    const uint32_t b = (uint32_t)(b0 + blockIdx.y);
    for (int q4 = threadIdx.x; q4 < (m + 3) / 4; q4 += blockDim.x) {
        uint32_t c[4] = {(uint32_t)q4, b, (uint32_t)t, stream};
        bs_philox(c, seed);
#pragma unroll
        for (int h = 0; h < 4; ++h)
            if (4 * q4 + h < m) atomicAdd(&hist[__umulhi(c[h], size)], 1);
    }
    __syncthreads();
    int32_t *__restrict__ row = w + (int64_t)blockIdx.y * ldw + (first - col0);
    for (uint32_t i = threadIdx.x; i < size; i += blockDim.x) row[i] = hist[i];
}

// keep byte of samples i0 .. i0 + nr - 1: every component of fine and coarse passes the basis transform (moments.hip, k_mask)
__global__ __launch_bounds__(256) void k_bs_keep(BasisParams bp, const double *__restrict__ f, const double *__restrict__ c, int64_t n,
                                                 int M, int64_t i0, int64_t nr, uint8_t *__restrict__ keep) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nr; i += (int64_t)gridDim.x * blockDim.x) {
        bool k = true;
        for (int m = 0; m < M; ++m) {
            bool k1, k2 = true;
            transform_value(bp, f[(int64_t)m * n + i0 + i], k1);
            if (c) transform_value(bp, c[(int64_t)m * n + i0 + i], k2);
            k = k && k1 && k2;
        }
        keep[i] = k ? 1 : 0;
    }
}

// keep byte of component m at samples i0 .. i0 + nr - 1, keep[m * ldk + i]: the fine and the coarse value pass component m's own
// transform (moments_multi.hip: the rule of a one-component chunk).  grid (sample blocks, components)
__global__ __launch_bounds__(256) void k_bs_keep_multi(const BasisParams *__restrict__ tab, const double *__restrict__ f,
                                                       const double *__restrict__ c, int64_t n, int M, int64_t i0, int64_t nr,
                                                       int64_t ldk, uint8_t *__restrict__ keep) {
    for (int m = blockIdx.y; m < M; m += gridDim.y) {
        const BasisParams bp = tab[m];
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nr; i += (int64_t)gridDim.x * blockDim.x) {
            bool k1, k2 = true;
            transform_value(bp, f[(int64_t)m * n + i0 + i], k1);
            if (c) transform_value(bp, c[(int64_t)m * n + i0 + i], k2);
            keep[(int64_t)m * ldk + i] = (k1 && k2) ? 1 : 0;
        }
    }
}

// ---- column layouts: what the two routes do not share ---------------------------------------------------------------------------
// k_bs_contract and k_bs_reduce work on the columns of the M components of one launch and ask a layout four things:
//   basis(m)         the BasisParams of component m
//   side_keep(s)     the byte the contraction stages in LDS for sample s of the range (the keep byte of the side count, if any)
//   kept(m, s, side) whether component m keeps sample s; side: the staged byte of s
//   width(), FLAG    columns per component; the first FLAG of them are a keep flag (1 for a kept sample), the others the terms d_r
//   the kept count and the totals: Count / store_count in the contraction, total / reduce_count in the reduction
// Both are passed by value and serve both kernels of a (range, component group).

// One basis and one mask for all components (mlmc_bootstrap_create): component m owns R columns, the kept count sum w keep is an
// integer sum on the side (workgroups of column block 0), totals [B][2 MR] (sum w d | sum w d^2) and counts [B].
struct BsSharedBasis {
    BasisParams bp;
    const uint8_t *keep;   // [range]: the AND over the components (k_bs_keep)
    int R, MR;
    int32_t *pcnt;         // partial counts [64-replicate tile][slice][64]
    double *tot;           // of the level
    int64_t *cnt;
    static constexpr int FLAG = 0;
    __device__ const BasisParams &basis(int) const { return bp; }
    __device__ int side_keep(int64_t s) const { return keep[s]; }
    __device__ bool kept(int, int64_t, int side) const { return side != 0; }
    __device__ int width() const { return R; }
    struct Count {
        int c = 0;
        __device__ void add(int w, int k) { c += w * k; }
    };
    __device__ void store_count(Count n, int lane, int wave) const {        // lanes l, l + 16, l + 32, l + 48 hold one replicate
        if (blockIdx.z != 0) return;
        int c = n.c;
        c += __shfl_xor(c, 16, 64);
        c += __shfl_xor(c, 32, 64);
        if (lane < 16) pcnt[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * BS_REPS + 16 * wave + lane] = c;
    }
    // where column j (its sum of squares: sq) of replicate b goes; null: nowhere
    __device__ double *total(int64_t b, int j, bool sq) const { return j < MR ? tot + b * 2 * MR + (sq ? MR + j : j) : nullptr; }
    __device__ void reduce_count(int nx, int64_t b_first, int reps) const {
        if (blockIdx.x != 0 || blockIdx.z != 0 || threadIdx.x >= BS_REPS) return;
        const int b = blockIdx.y * BS_REPS + threadIdx.x;
        if (b >= reps) return;
        int64_t s = 0;
        for (int x = 0; x < nx; ++x) s += pcnt[((int64_t)blockIdx.y * nx + x) * BS_REPS + threadIdx.x];
        cnt[b_first + b] += s;
    }
};

// A basis and a mask per component (mlmc_bootstrap_create_multi), for a group of components: tab, keep and tot point at the group's
// first one.  Component m owns K + 1 columns, m (K + 1) = its keep flag, m (K + 1) + 1 + k = d_k.  The flag column rides through
// the same MFMAs: sum w keep is a sum of integers below 2^53, exact in fp64 in any order, so the kept count of every (replicate,
// component) comes out as an exact integer with the sums.  Totals [B][ld_tot], per component (sum w d [K] | sum w d^2 [K] | kept
// count); the sum of squares of a flag column is not used.
struct BsPerComponent {
    const BasisParams *tab;   // [M]
    const uint8_t *keep;      // [M][ldk] (k_bs_keep_multi)
    int64_t ldk;
    int K, cols;              // cols = M (K + 1)
    double *tot;              // of the level
    int64_t ld_tot;
    static constexpr int FLAG = 1;
    __device__ const BasisParams &basis(int m) const { return tab[m]; }
    __device__ int side_keep(int64_t) const { return 0; }
    __device__ bool kept(int m, int64_t s, int) const { return keep[(int64_t)m * ldk + s] != 0; }
    __device__ int width() const { return K + 1; }
    struct Count {
        __device__ void add(int, int) {}
    };
    __device__ void store_count(Count, int, int) const {}
    __device__ double *total(int64_t b, int j, bool sq) const {
        const int m = j / (K + 1), q = j % (K + 1);
        if (j >= cols || (sq && q == 0)) return nullptr;
        double *t = tot + b * ld_tot + (int64_t)m * (2 * K + 1);
        return sq ? t + K + q - 1 : t + (q ? q - 1 : 2 * K);
    }
    __device__ void reduce_count(int, int64_t, int) const {}
};

// The contraction of M components (fine / coarse point at the first one).  grid (slices of BS_SW samples of the range, 64-replicate
// tiles, column blocks of JB = 16 JT columns; a block may straddle components).
// Per batch of BS_KB samples: the weights [64][KB] -> LDS, Phi [KB][JB] (flags and d of the block's columns; 0 where the column's
// component drops the sample; a wave handles one component per trip: KB = 64 samples) -> LDS, then each wave runs KB / 4 k-steps of
// 2 JT MFMAs: sum w d and sum w d^2 for its 16 replicates.  Partial rows: [64][2 JB] per workgroup.
template <int KIND, bool PAIR, int JT, class Layout>
__global__ __launch_bounds__(256) void k_bs_contract(Layout lay, const double *__restrict__ fine, const double *__restrict__ coarse,
                                                     int64_t n, int M, int64_t i0, int64_t nr, const int32_t *__restrict__ W,
                                                     int64_t ldw, int reps, double *__restrict__ partials) {
    constexpr int JB = 16 * JT;
    constexpr int KB = BS_KB;
    constexpr int WS = KB + 4;                       // rows of 16 replicates x 4 samples hit 64 distinct banks
    constexpr int PS = 32 * ((JB + 31) / 32) + 16;   // == 16 (mod 32): two k-rows of a fragment read in distinct bank halves
    __shared__ int32_t wl[BS_REPS * WS];
    __shared__ double ph[KB * PS];
    __shared__ uint8_t kp[KB];                       // Layout::side_keep of the batch

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cw = lay.width();
    const int j0 = blockIdx.z * JB;
    const int m_lo = j0 / cw, m_hi = std::min(M - 1, (j0 + JB - 1) / cw);
    const int ncomp = m_hi - m_lo + 1;
    const int y0 = blockIdx.y * BS_REPS;
    const int64_t s_begin = (int64_t)blockIdx.x * BS_SW, s_end = std::min(nr, s_begin + BS_SW);

    v4f64 a1[JT], a2[JT];
#pragma unroll
    for (int J = 0; J < JT; ++J) {
        a1[J] = (v4f64){0.0, 0.0, 0.0, 0.0};
        a2[J] = (v4f64){0.0, 0.0, 0.0, 0.0};
    }
    typename Layout::Count cnt;
    for (int64_t s0 = s_begin; s0 < s_end; s0 += KB) {
        const int kb = (int)std::min((int64_t)KB, s_end - s0);
        for (int e = threadIdx.x; e < BS_REPS * KB; e += 256) {
            const int r = e / KB, k = e % KB;
            wl[r * WS + k] = (y0 + r < reps && k < kb) ? W[(int64_t)(y0 + r) * ldw + s0 + k] : 0;
        }
        if (threadIdx.x < KB) kp[threadIdx.x] = (int)threadIdx.x < kb ? lay.side_keep(s0 + threadIdx.x) : 0;
        for (int e = threadIdx.x; e < KB * JB; e += 256) ph[(e / JB) * PS + e % JB] = 0.0;
        __syncthreads();
        for (int it = threadIdx.x; it < KB * ncomp; it += 256) {
            const int k = it % KB, m = m_lo + it / KB;
            if (k >= kb || !lay.kept(m, s0 + k, kp[k])) continue;
            const BasisParams bp = lay.basis(m);
            const int64_t idx = (int64_t)m * n + i0 + s0 + k;
            bool kf, kc = true;
            const double tf = transform_value(bp, fine[idx], kf);
            const double tc = PAIR ? transform_value(bp, coarse[idx], kc) : 0.0;
            TermGen<KIND> gf, gc;
            gf.init(tf, 1.0, bp);
            if (PAIR) gc.init(tc, 1.0, bp);
            const int c0 = m * cw - j0;                                  // block column of the component's first column: < JB, may be < 0
            if (Layout::FLAG && c0 >= 0) ph[k * PS + c0] = 1.0;
            const int t0 = c0 + Layout::FLAG;                            // ... of its term 0
            const int rb = -t0, re = std::min(cw - Layout::FLAG, JB - t0);   // the block holds terms max(rb, 0) .. re - 1 of component m
            for (int r = 0; r < re; ++r) {
                double d = gf.next(r);
                if (PAIR) d -= gc.next(r);
                if (r >= rb) ph[k * PS + t0 + r] = d;
            }
        }
        __syncthreads();
        const int arow = (16 * wave + (lane & 15)) * WS;
#pragma unroll 4
        for (int kk = 0; kk < KB / 4; ++kk) {
            const int k = 4 * kk + (lane >> 4);
            const int wv = wl[arow + k];
            cnt.add(wv, kp[k]);
            const double a = (double)wv;
#pragma unroll
            for (int J = 0; J < JT; ++J) {
                const double bv = ph[k * PS + 16 * J + (lane & 15)];
                a1[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, a1[J], 0, 0, 0);
                a2[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv * bv, a2[J], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // f64 MFMA C/D layout: register r of lane l holds (row l / 16 + 4 r, column l % 16) of the tile
    double *__restrict__ prow = partials + (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (BS_REPS * 2 * JB);
#pragma unroll
    for (int J = 0; J < JT; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rep = 16 * wave + (lane >> 4) + 4 * r, col = 16 * J + (lane & 15);
            prow[rep * 2 * JB + col] = a1[J][r];
            prow[rep * 2 * JB + JB + col] = a2[J][r];
        }
    lay.store_count(cnt, lane, wave);
}

// Level totals += the partial rows of one contraction launch, summed over the slices in a fixed order.
// grid (ceil(64 * 2 JB / 256), 64-replicate tiles, column blocks)
template <class Layout>
__global__ __launch_bounds__(256) void k_bs_reduce(Layout lay, const double *__restrict__ partials, int nx, int JB, int64_t b_first,
                                                   int reps) {
    const int row = BS_REPS * 2 * JB;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < row) {
        const int rep = e / (2 * JB), c = e % (2 * JB);
        const int b = blockIdx.y * BS_REPS + rep;
        double *dst = b < reps ? lay.total(b_first + b, blockIdx.z * JB + c % JB, c >= JB) : nullptr;
        if (dst) {
            const double *__restrict__ p = partials + ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * nx * row + e;
            double s = 0.0;
            for (int x = 0; x < nx; ++x) s += p[(int64_t)x * row];
            *dst += s;
        }
    }
    lay.reduce_count(nx, b_first, reps);
}

// ---- host side ----------------------------------------------------------------------------
struct BsScratch {              // one per accumulator / weights call: sized by the budgets above, never by B x n
    int32_t *counts = nullptr;   // [rows][n_tiles]
    int32_t *w = nullptr;        // [BG][nr]
    double *part = nullptr;
    int32_t *pcnt = nullptr;
    uint8_t *keep = nullptr;
};

static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// pass A for replicates b0 .. b0 + nb - 1 (sizes: device-readable) into counts [nb][n_tiles] (zeroed here)
static int launch_tile_counts(int64_t n, int64_t nb, const int64_t *d_sizes, int64_t max_size, int64_t b0, uint64_t seed,
                              uint32_t stream, int32_t *counts) {
    const int64_t n_tiles = cdiv(n, BS_TILE);
    MLMC_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)(nb * n_tiles), rt().stream));
    if (max_size <= 0) return 0;
    const int64_t nseg = cdiv(n_tiles, BS_SEG_TILES);
    // enough positions per workgroup that the flush of its histogram (<= BS_SEG_TILES integer atomics) stays a small part
    const int64_t pairs_per_wg = std::max<int64_t>(4096, 4 * std::min<int64_t>(n_tiles, BS_SEG_TILES));
    const int64_t gx = cdiv(cdiv(max_size, 2), pairs_per_wg);
    hipLaunchKernelGGL(k_bs_tile_counts, dim3((unsigned)gx, (unsigned)nb, (unsigned)nseg), dim3(256), 0, rt().stream, n, n_tiles,
                       d_sizes, b0, pairs_per_wg, seed, stream, counts);
    MLMC_HIP_CHECK(hipGetLastError());
    return 0;
}

static int launch_expand(int64_t n, int64_t nb, int64_t t_first, int64_t nt, const int32_t *counts, int64_t b0, uint64_t seed,
                         uint32_t stream, int32_t *w, int64_t ldw, int64_t col0) {
    if (nt <= 0 || nb <= 0) return 0;
    hipLaunchKernelGGL(k_bs_expand, dim3((unsigned)nt, (unsigned)nb), dim3(256), 0, rt().stream, n, cdiv(n, BS_TILE), t_first,
                       counts, b0, seed, stream, w, ldw, col0);
    MLMC_HIP_CHECK(hipGetLastError());
    return 0;
}

static std::string check_sizes(const char *fn, const int64_t *sizes, int64_t nb, int64_t n) {
    for (int64_t b = 0; b < nb; ++b)
        if (sizes[b] < 0 || sizes[b] > n)
            return std::string(fn) + ": sizes[" + std::to_string(b) + "] = " + std::to_string(sizes[b]) + " is outside [0, n = " +
                   std::to_string(n) + "]";
    return std::string();
}

}  // namespace mlmc

struct mlmc_bootstrap {
    const mlmc_basis *basis = nullptr;
    int M = 0, L = 0, R = 0, MR = 0;
    int64_t B = 0;
    double *d_tot = nullptr;              // [L][B][2 MR]: sum w d | sum w d^2 (Legendre: scaled terms, finalize applies scale_c)
    int64_t *d_cnt = nullptr;             // [L][B]
    mlmc::BsScratch sc;
    std::vector<int64_t *> h_sizes;       // pinned [B] blocks, one per accumulated chunk since the last finalize / reset
    size_t sizes_used = 0;
    std::vector<hipEvent_t> ev;           // timing pairs (FLAG_TIMING), with their kind: 0 = RNG, 1 = contraction
    std::vector<int> ev_kind;
    size_t ev_used = 0;
    double ms_rng = 0, ms_contract = 0;
    int64_t flops = 0;
    int64_t keep_tiles = 0;               // tiles per sample range the keep bytes allow
    // per-component handle (mlmc_bootstrap_create_multi): R = K, totals [L][B][M (2 K + 1)], no d_cnt
    bool multi = false;
    std::vector<const mlmc_basis *> bases;
    mlmc::BasisParams *d_tab = nullptr;   // [M]
    uint8_t *d_keep_m = nullptr;          // [M][keep_tiles * BS_TILE]
    // component-covariance handle (mlmc_bootstrap_create_xcov): no basis, totals [L][B][C], C = 1 + M + M (M + 1) / 2, no d_cnt
    bool xcov = false;
    int64_t C = 0;
    double *d_shift = nullptr;            // [M]: uploaded by reset from shift_host (mlmc_bootstrap_set_shift)
    std::vector<double> shift_host;
    int64_t pushes = 0;                   // chunks accumulated since the last reset
    size_t tot_bytes() const {
        if (xcov) return sizeof(double) * (size_t)L * (size_t)B * (size_t)C;
        return sizeof(double) * (size_t)L * (size_t)B * (multi ? (size_t)M * (2 * (size_t)R + 1) : 2 * (size_t)MR);
    }
};

namespace mlmc {

static int bs_time(mlmc_bootstrap *a, int kind, bool end) {
    if (!(rt().flags & 1)) return 0;
    if (!end) {
        if (a->ev_used + 2 > a->ev.size()) {
            hipEvent_t e0, e1;
            MLMC_HIP_CHECK(hipEventCreate(&e0));
            MLMC_HIP_CHECK(hipEventCreate(&e1));
            a->ev.push_back(e0);
            a->ev.push_back(e1);
            a->ev_kind.push_back(0);
            a->ev_kind.push_back(0);
        }
        a->ev_kind[a->ev_used] = kind;
        MLMC_HIP_CHECK(hipEventRecord(a->ev[a->ev_used], rt().stream));
        return 0;
    }
    MLMC_HIP_CHECK(hipEventRecord(a->ev[a->ev_used + 1], rt().stream));
    a->ev_used += 2;
    return 0;
}

static int bs_time_collect(mlmc_bootstrap *a) {
    for (size_t i = 0; i + 1 < a->ev_used; i += 2) {
        float ms = 0.f;
        MLMC_HIP_CHECK(hipEventElapsedTime(&ms, a->ev[i], a->ev[i + 1]));
        (a->ev_kind[i] ? a->ms_contract : a->ms_rng) += ms;
    }
    a->ev_used = 0;
    return 0;
}

static int bs_scratch_alloc(BsScratch &sc) {
    MLMC_HIP_CHECK(hipMalloc((void **)&sc.counts, BS_COUNTS_BYTES));
    MLMC_HIP_CHECK(hipMalloc((void **)&sc.w, BS_W_BYTES));
    MLMC_HIP_CHECK(hipMalloc((void **)&sc.part, BS_PART_BYTES));
    MLMC_HIP_CHECK(hipMalloc((void **)&sc.pcnt, (size_t)BS_NY_MAX * BS_TPR_MAX * (BS_TILE / BS_SW) * BS_REPS * 4));
    MLMC_HIP_CHECK(hipMalloc((void **)&sc.keep, (size_t)BS_TPR_MAX * BS_TILE));
    return 0;
}

static void bs_scratch_free(BsScratch &sc) {
    if (sc.counts) (void)hipFree(sc.counts);
    if (sc.w) (void)hipFree(sc.w);
    if (sc.part) (void)hipFree(sc.part);
    if (sc.pcnt) (void)hipFree(sc.pcnt);
    if (sc.keep) (void)hipFree(sc.keep);
    sc = BsScratch();
}

// (kind, pair, JT) -> the instantiation of k_bs_contract for a layout
template <class Layout>
using BsContractFn = void (*)(Layout, const double *, const double *, int64_t, int, int64_t, int64_t, const int32_t *, int64_t, int,
                              double *);

template <class L>
static BsContractFn<L> bs_contract_kernel(int kind, bool pair, int JT) {
    static const BsContractFn<L> fn[3][2][3] = {
        {{k_bs_contract<MLMC_LEGENDRE, false, 1, L>, k_bs_contract<MLMC_LEGENDRE, false, 2, L>, k_bs_contract<MLMC_LEGENDRE, false, 4, L>},
         {k_bs_contract<MLMC_LEGENDRE, true, 1, L>, k_bs_contract<MLMC_LEGENDRE, true, 2, L>, k_bs_contract<MLMC_LEGENDRE, true, 4, L>}},
        {{k_bs_contract<MLMC_MONOMIAL, false, 1, L>, k_bs_contract<MLMC_MONOMIAL, false, 2, L>, k_bs_contract<MLMC_MONOMIAL, false, 4, L>},
         {k_bs_contract<MLMC_MONOMIAL, true, 1, L>, k_bs_contract<MLMC_MONOMIAL, true, 2, L>, k_bs_contract<MLMC_MONOMIAL, true, 4, L>}},
        {{k_bs_contract<MLMC_FOURIER, false, 1, L>, k_bs_contract<MLMC_FOURIER, false, 2, L>, k_bs_contract<MLMC_FOURIER, false, 4, L>},
         {k_bs_contract<MLMC_FOURIER, true, 1, L>, k_bs_contract<MLMC_FOURIER, true, 2, L>, k_bs_contract<MLMC_FOURIER, true, 4, L>}}};
    return fn[kind == MLMC_LEGENDRE ? 0 : (kind == MLMC_MONOMIAL ? 1 : 2)][pair][JT / 2];
}

// the contraction of one (replicate group, sample range, component group) and its reduction into the totals the layout names
template <class Layout>
static int bs_contract_reduce(const Layout &lay, int kind, int JT, dim3 grid, const double *f, const double *c, int64_t n, int M,
                              int64_t i0, int64_t len, const BsScratch &sc, int64_t ldw, int64_t g, int ng) {
    const int JB = 16 * JT;
    hipLaunchKernelGGL(bs_contract_kernel<Layout>(kind, c != nullptr, JT), grid, dim3(256), 0, rt().stream, lay, f, c, n, M, i0, len,
                       sc.w, ldw, ng, sc.part);
    MLMC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_bs_reduce<Layout>, dim3((unsigned)cdiv(BS_REPS * 2 * JB, 256), grid.y, grid.z), dim3(256), 0, rt().stream, lay,
                       sc.part, (int)grid.x, JB, g, ng);
    MLMC_HIP_CHECK(hipGetLastError());
    return 0;
}

// components per group of the per-component route: at most BS_MAX_COLS group columns of K + 1 each
static int64_t bs_group_comps(int64_t M, int64_t K) { return std::min<int64_t>(M, std::max<int64_t>(1, BS_MAX_COLS / (K + 1))); }

// How a chunk of n samples is cut: column blocks of 16 JT, sample ranges of nr, replicate groups of BG.  JT and nr are functions
// of n, the columns of the largest component group and the tiles the keep bytes allow -- never of B: a replicate's summation
// order must not depend on it.
struct BsPlan {
    int JT;
    int64_t nr, BG;
};

static BsPlan bs_plan(int64_t n, int64_t B, int64_t cols, int64_t keep_tiles) {
    const int JT = cols <= 16 ? 1 : (cols <= 32 ? 2 : 4);
    const int JB = 16 * JT;
    const int64_t ncb = cdiv(cols, JB);
    const int64_t n_tiles = cdiv(n, BS_TILE);
    const size_t pwb = (size_t)BS_REPS * 2 * JB * sizeof(double);      // partial row block of one workgroup
    constexpr int SPT = BS_TILE / BS_SW;                                 // slices per tile
    const int64_t tpr = std::max<int64_t>(1, std::min<int64_t>({n_tiles, (int64_t)BS_TPR_MAX, keep_tiles,
                                                                 (int64_t)(BS_PART_BYTES / (pwb * SPT * ncb))}));
    const int64_t nx_full = tpr * SPT;
    int64_t ny = std::min<int64_t>({cdiv(B, BS_REPS), (int64_t)BS_NY_MAX, (int64_t)(BS_PART_BYTES / (pwb * nx_full * ncb)),
                                    (int64_t)(BS_COUNTS_BYTES / (4 * (size_t)BS_REPS * n_tiles))});
    ny = std::max<int64_t>(ny, 1);
    return BsPlan{JT, tpr * BS_TILE, ny * BS_REPS};
}

// The walk over one chunk that every kind of handle shares (ds: the device view of the pinned sizes): replicates in groups of
// p.BG, samples in ranges of p.nr; per group pass A, per (group, range) pass B into the weight slab and then
// contract(g, ng, i0, len) -- the keep bytes, the contractions and their reductions -- between the contraction's timing events.
template <class F>
static int bs_walk(mlmc_bootstrap *a, int64_t n, const BsPlan &p, const int64_t *sizes, const int64_t *ds, uint64_t seed, uint32_t stream,
                   F contract) {
    const int64_t B = a->B, nr = p.nr, BG = p.BG;
    for (int64_t g = 0; g < B; g += BG) {
        const int64_t ng = std::min(BG, B - g);
        const int64_t mx = *std::max_element(sizes + g, sizes + g + ng);
        if (int rc = bs_time(a, 0, false)) return rc;
        if (int rc = launch_tile_counts(n, ng, ds + g, mx, g, seed, stream, a->sc.counts)) return rc;
        if (int rc = bs_time(a, 0, true)) return rc;
        for (int64_t i0 = 0; i0 < n; i0 += nr) {
            const int64_t len = std::min(nr, n - i0);
            if (int rc = bs_time(a, 0, false)) return rc;
            if (int rc = launch_expand(n, ng, i0 / BS_TILE, cdiv(len, BS_TILE), a->sc.counts, g, seed, stream, a->sc.w, nr, i0)) return rc;
            if (int rc = bs_time(a, 0, true)) return rc;
            if (int rc = bs_time(a, 1, false)) return rc;
            if (int rc = contract(g, ng, i0, len)) return rc;
            if (int rc = bs_time(a, 1, true)) return rc;
        }
    }
    return 0;
}

// MFMA batches of BS_KB samples that the workgroups of one replicate tile and column block run over a range of len samples
static int64_t bs_batches(int64_t len) {
    const int64_t nx = cdiv(len, BS_SW);
    return (nx - 1) * (BS_SW / BS_KB) + cdiv(len - (nx - 1) * BS_SW, BS_KB);
}

// One chunk of a moments handle (mlmc_bootstrap_accum has checked the arguments).  Per (replicate group, sample range): the keep
// bytes once, then per component group the contraction and its fixed-order reduction.  The shared-basis handle has one group of
// all M components.
static int bs_accum(mlmc_bootstrap *a, int32_t level, const double *fine, const double *coarse, int64_t n, const int64_t *sizes,
                    const int64_t *ds, uint64_t seed, uint32_t stream) {
    const int64_t B = a->B, M = a->M, R = a->R;
    const int64_t cw = a->multi ? R + 1 : R;                             // columns per component
    const int64_t mg = a->multi ? bs_group_comps(M, R) : M;
    const BsPlan p = bs_plan(n, B, mg * cw, a->keep_tiles);
    const int JT = p.JT, JB = 16 * JT;
    const int64_t nr = p.nr;
    const int64_t ldk = a->keep_tiles * BS_TILE;
    const int64_t ld_tot = a->multi ? M * (2 * R + 1) : 2 * M * R;
    const BasisParams bp = a->basis->p;
    double *tot = a->d_tot + (size_t)level * B * ld_tot;
    return bs_walk(a, n, p, sizes, ds, seed, stream, [&](int64_t g, int64_t ng, int64_t i0, int64_t len) -> int {
        const int64_t nyg = cdiv(ng, BS_REPS), nx = cdiv(len, BS_SW);
        if (a->multi)
            hipLaunchKernelGGL(k_bs_keep_multi, dim3((unsigned)cdiv(len, 256), (unsigned)M), dim3(256), 0, rt().stream, a->d_tab, fine,
                               coarse, n, (int)M, i0, len, ldk, a->d_keep_m);
        else
            hipLaunchKernelGGL(k_bs_keep, dim3((unsigned)cdiv(len, 256)), dim3(256), 0, rt().stream, bp, fine, coarse, n, (int)M, i0,
                               len, a->sc.keep);
        MLMC_HIP_CHECK(hipGetLastError());
        for (int64_t m0 = 0; m0 < M; m0 += mg) {
            const int64_t mc = std::min(mg, M - m0);
            const int cols = (int)(mc * cw);
            const int64_t ncb = cdiv(cols, JB);
            const dim3 grid((unsigned)nx, (unsigned)nyg, (unsigned)ncb);
            const double *f = fine + m0 * n, *c = coarse ? coarse + m0 * n : nullptr;
            const int rc = a->multi
                ? bs_contract_reduce(BsPerComponent{a->d_tab + m0, a->d_keep_m + m0 * ldk, ldk, (int)R, cols, tot + m0 * (2 * R + 1), ld_tot},
                                     bp.kind, JT, grid, f, c, n, (int)mc, i0, len, a->sc, nr, g, (int)ng)
                : bs_contract_reduce(BsSharedBasis{bp, a->sc.keep, (int)R, cols, a->sc.pcnt, tot, a->d_cnt + (size_t)level * B},
                                     bp.kind, JT, grid, f, c, n, (int)mc, i0, len, a->sc, nr, g, (int)ng);
            if (rc) return rc;
            // executed matrix-core flops: every batch of every workgroup runs KB / 4 k-steps of 2 JT MFMAs per wave
            a->flops += bs_batches(len) * nyg * ncb * 4 * (BS_KB / 4) * 2 * JT * (int64_t)(16 * 16 * 4 * 2);
        }
        return 0;
    });
}

// ---- component covariance of the replicates (mlmc_bootstrap_create_xcov) -------------------------------------------------------
// Columns of a replicate's row of totals: 0 = the kept count (a flag column, exact as in BsPerComponent), 1 + m = the first
// moment of component m, 1 + M + p = product pair p = (i, j), i <= j, row-major over the upper triangle (row i starts at
// i M - i (i - 1) / 2).
constexpr int BSX_MAX_M = 1024;

static int64_t bsx_cols(int64_t M) { return 1 + M + M * (M + 1) / 2; }

// column -> (ci, cj): (-1, -1) the flag, (m, -1) a first moment, (i, j) a product pair, (-2, -2) past the last column
__device__ __forceinline__ void bsx_column(int64_t col, int M, int64_t C, int &ci, int &cj) {
    if (col >= C) { ci = cj = -2; return; }
    if (col == 0) { ci = cj = -1; return; }
    if (col <= M) { ci = (int)col - 1; cj = -1; return; }
    const int64_t p = col - 1 - M;
    const double h = 2.0 * M + 1.0;
    int i = (int)((h - sqrt(h * h - 8.0 * (double)p)) * 0.5);          // a guess; the two loops make it exact
    i = std::max(0, std::min(i, M - 1));
    while (i > 0 && (int64_t)i * M - (int64_t)i * (i - 1) / 2 > p) --i;
    while (i + 1 < M && (int64_t)(i + 1) * M - (int64_t)(i + 1) * i / 2 <= p) ++i;
    ci = i;
    cj = i + (int)(p - ((int64_t)i * M - (int64_t)i * (i - 1) / 2));
}

// keep byte of samples i0 .. i0 + nr - 1: no NaN among the M fine and M coarse values (the rule of k_xcov_mask)
__global__ __launch_bounds__(256) void k_bs_xcov_keep(const double *__restrict__ f, const double *__restrict__ c, int64_t n, int M,
                                                      int64_t i0, int64_t nr, uint8_t *__restrict__ keep) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nr; i += (int64_t)gridDim.x * blockDim.x) {
        bool k = true;
        for (int m = 0; m < M; ++m) {
            const double v = f[(int64_t)m * n + i0 + i];
            k = k && !(v != v);
            if (c) {
                const double u = c[(int64_t)m * n + i0 + i];
                k = k && !(u != u);
            }
        }
        keep[i] = k ? 1 : 0;
    }
}

// The contraction of the columns col0 + blockIdx.z * JB .. of one (replicate group, sample range): grid as k_bs_contract (slices of
// BS_SW samples, 64-replicate tiles, column blocks of JB = 16 JT).  Per batch of BS_KB samples: the weights [64][KB] -> LDS; Phi
// [JB][KB] -> LDS, every element one flag, one shifted difference or one product pair, its factors read from global memory (a
// wave owns one column per trip, its 64 lanes the 64 samples: coalesced along the samples), the shift subtracted and a dropped
// sample written as 0.0; then each wave runs KB / 4 k-steps of JT MFMAs for its 16 replicates.  Partial rows: [64][JB] per
// workgroup.
template <bool PAIR, int JT>
__global__ __launch_bounds__(256) void k_bs_xcov_contract(const double *__restrict__ fine, const double *__restrict__ coarse,
                                                          const double *__restrict__ shift, const uint8_t *__restrict__ keep, int64_t n,
                                                          int M, int64_t C, int64_t col0, int64_t i0, int64_t nr,
                                                          const int32_t *__restrict__ W, int64_t ldw, int reps,
                                                          double *__restrict__ partials) {
    constexpr int JB = 16 * JT;
    constexpr int KB = BS_KB;
    constexpr int WS = KB + 4;                       // as k_bs_contract
    constexpr int KS = KB + 2;                       // == 2 (mod 32): the fragment reads hit distinct bank pairs (xcov.hip)
    __shared__ int32_t wl[BS_REPS * WS];
    __shared__ double ph[JB * KS];
    __shared__ int cpi[JB], cpj[JB];
    __shared__ double sai[JB], saj[JB];              // the shifts of the column's two components

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y0 = blockIdx.y * BS_REPS;
    const int64_t s_begin = (int64_t)blockIdx.x * BS_SW, s_end = std::min(nr, s_begin + BS_SW);
    if (threadIdx.x < JB) {
        int ci, cj;
        bsx_column(col0 + (int64_t)blockIdx.z * JB + threadIdx.x, M, C, ci, cj);
        cpi[threadIdx.x] = ci;
        cpj[threadIdx.x] = cj;
        sai[threadIdx.x] = ci >= 0 ? shift[ci] : 0.0;
        saj[threadIdx.x] = cj >= 0 ? shift[cj] : 0.0;
    }
    __syncthreads();

    v4f64 acc[JT];
#pragma unroll
    for (int J = 0; J < JT; ++J) acc[J] = (v4f64){0.0, 0.0, 0.0, 0.0};
    for (int64_t s0 = s_begin; s0 < s_end; s0 += KB) {
        const int kb = (int)std::min((int64_t)KB, s_end - s0);
        for (int e = threadIdx.x; e < BS_REPS * KB; e += 256) {
            const int r = e / KB, k = e % KB;
            wl[r * WS + k] = (y0 + r < reps && k < kb) ? W[(int64_t)(y0 + r) * ldw + s0 + k] : 0;
        }
        {
            // Every load is unconditional (a flag or first-moment column reads component 0 in place of the factor it does not
            // have, a lane past the batch reads the batch's first sample) and NH elements' loads are issued before the first use:
            // behind a branch they would wait for each other, one memory latency per element.
            constexpr int NE = JB / 4, NH = NE < 8 ? NE : 8;             // elements per thread and batch; ... loaded together
            const bool kept = lane < kb && keep[s0 + lane] != 0;
            const int64_t at = i0 + s0 + (lane < kb ? lane : 0);         // < n
#pragma unroll
            for (int h = 0; h < NE; h += NH) {
                double fi[NH], fj[NH], gi[NH], gj[NH];
#pragma unroll
                for (int t = 0; t < NH; ++t) {
                    const int jj = wave + 4 * (h + t);
                    const int64_t oi = (int64_t)std::max(cpi[jj], 0) * n + at, oj = (int64_t)std::max(cpj[jj], 0) * n + at;
                    fi[t] = fine[oi];
                    fj[t] = fine[oj];
                    gi[t] = PAIR ? coarse[oi] : 0.0;
                    gj[t] = PAIR ? coarse[oj] : 0.0;
                }
#pragma unroll
                for (int t = 0; t < NH; ++t) {
                    const int jj = wave + 4 * (h + t);
                    const int ci = cpi[jj], cj = cpj[jj];
                    const double ai = sai[jj], aj = saj[jj];
                    const double xi = fi[t] - ai, yi = gi[t] - ai;
                    double v;
                    if (cj >= 0) {
                        v = xi * (fj[t] - aj);
                        if (PAIR) v -= yi * (gj[t] - aj);
                    } else {
                        v = PAIR ? xi - yi : xi;
                    }
                    if (ci == -1) v = 1.0;
                    ph[jj * KS + lane] = (kept && ci != -2) ? v : 0.0;   // a dropped sample: 0.0, never a product with a NaN
                }
            }
        }
        __syncthreads();
        const int arow = (16 * wave + (lane & 15)) * WS;
#pragma unroll 4
        for (int kk = 0; kk < KB / 4; ++kk) {
            const int k = 4 * kk + (lane >> 4);
            const double a = (double)wl[arow + k];
#pragma unroll
            for (int J = 0; J < JT; ++J)
                acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, ph[(16 * J + (lane & 15)) * KS + k], acc[J], 0, 0, 0);
        }
        __syncthreads();
    }
    // f64 MFMA C/D layout: register r of lane l holds (row l / 16 + 4 r, column l % 16) of the tile
    double *__restrict__ prow = partials + (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (BS_REPS * JB);
#pragma unroll
    for (int J = 0; J < JT; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) prow[(16 * wave + (lane >> 4) + 4 * r) * JB + 16 * J + (lane & 15)] = acc[J][r];
}

// Level totals [B][C] += the partial rows of one k_bs_xcov_contract launch, summed over the slices in a fixed order.
// grid (ceil(64 JB / 256), 64-replicate tiles, column blocks)
__global__ __launch_bounds__(256) void k_bs_xcov_reduce(const double *__restrict__ partials, int nx, int JB, int64_t C, int64_t col0,
                                                        int64_t b_first, int reps, double *__restrict__ tot) {
    const int row = BS_REPS * JB;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= row) return;
    const int b = blockIdx.y * BS_REPS + e / JB;
    const int64_t col = col0 + (int64_t)blockIdx.z * JB + e % JB;
    if (b >= reps || col >= C) return;
    const double *__restrict__ p = partials + ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * nx * row + e;
    double s = 0.0;
    for (int x = 0; x < nx; ++x) s += p[(int64_t)x * row];
    tot[(b_first + b) * C + col] += s;
}

using BsXcovFn = void (*)(const double *, const double *, const double *, const uint8_t *, int64_t, int, int64_t, int64_t, int64_t,
                          int64_t, const int32_t *, int64_t, int, double *);

static BsXcovFn bs_xcov_kernel(bool pair, int JT) {
    static const BsXcovFn fn[2][3] = {{k_bs_xcov_contract<false, 1>, k_bs_xcov_contract<false, 2>, k_bs_xcov_contract<false, 4>},
                                      {k_bs_xcov_contract<true, 1>, k_bs_xcov_contract<true, 2>, k_bs_xcov_contract<true, 4>}};
    return fn[pair][JT / 2];
}

// One chunk of a component-covariance handle: the walk of bs_accum; per (group, range) the keep bytes once, then per group of at
// most BS_MAX_COLS columns the contraction and its reduction.
static int bs_accum_xcov(mlmc_bootstrap *a, int32_t level, const double *fine, const double *coarse, int64_t n, const int64_t *sizes,
                         const int64_t *ds, uint64_t seed, uint32_t stream) {
    const int64_t B = a->B, M = a->M, C = a->C;
    const BsPlan p = bs_plan(n, B, std::min<int64_t>(C, BS_MAX_COLS), a->keep_tiles);
    const int JT = p.JT, JB = 16 * JT;
    const int64_t nr = p.nr;
    double *tot = a->d_tot + (size_t)level * B * C;
    const BsXcovFn kernel = bs_xcov_kernel(coarse != nullptr, JT);
    return bs_walk(a, n, p, sizes, ds, seed, stream, [&](int64_t g, int64_t ng, int64_t i0, int64_t len) -> int {
        const int64_t nyg = cdiv(ng, BS_REPS), nx = cdiv(len, BS_SW);
        hipLaunchKernelGGL(k_bs_xcov_keep, dim3((unsigned)cdiv(len, 256)), dim3(256), 0, rt().stream, fine, coarse, n, (int)M, i0, len,
                           a->sc.keep);
        MLMC_HIP_CHECK(hipGetLastError());
        for (int64_t c0 = 0; c0 < C; c0 += BS_MAX_COLS) {
            const int64_t ncb = cdiv(std::min<int64_t>(BS_MAX_COLS, C - c0), JB);
            const dim3 grid((unsigned)nx, (unsigned)nyg, (unsigned)ncb);
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, rt().stream, fine, coarse, a->d_shift, a->sc.keep, n, (int)M, C, c0, i0, len,
                               a->sc.w, nr, (int)ng, a->sc.part);
            MLMC_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_bs_xcov_reduce, dim3((unsigned)cdiv(BS_REPS * JB, 256), grid.y, grid.z), dim3(256), 0, rt().stream,
                               a->sc.part, (int)nx, JB, C, c0, g, (int)ng, tot);
            MLMC_HIP_CHECK(hipGetLastError());
            // executed matrix-core flops: every batch of every workgroup runs KB / 4 k-steps of JT MFMAs per wave
            a->flops += bs_batches(len) * nyg * ncb * 4 * (BS_KB / 4) * JT * (int64_t)(16 * 16 * 4 * 2);
        }
        return 0;
    });
}

// what both create functions check first (e: the entry point's name)
static int bs_create_check(const std::string &e, int32_t n_levels, int64_t B) {
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (n_levels < 1 || n_levels > 2047) return fail(e + ": n_levels = " + std::to_string(n_levels) + " (must be in 1 .. 2047)");
    if (B < 1 || B > (int64_t)INT32_MAX) return fail(e + ": B = " + std::to_string(B) + " (must be in 1 .. 2^31 - 1)");
    return 0;
}

}  // namespace mlmc

extern "C" int mlmc_bootstrap_weights(int64_t n, int64_t b0, int64_t nb, const int64_t *sizes, uint64_t seed, uint32_t stream,
                                      int32_t *w_out) {
    MLMC_API_GUARD;
    using namespace mlmc;
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (!sizes || !w_out) return fail("mlmc_bootstrap_weights: null argument (sizes, w_out)");
    if (n < 1 || n > BS_MAX_N)
        return fail("mlmc_bootstrap_weights: n = " + std::to_string(n) + " (must be in 1 .. " + std::to_string(BS_MAX_N) + ")");
    if (b0 < 0 || nb < 1 || b0 + nb > (int64_t)UINT32_MAX)
        return fail("mlmc_bootstrap_weights: replicates b0 = " + std::to_string(b0) + ", nb = " + std::to_string(nb) +
                    " (need b0 >= 0, nb >= 1, b0 + nb < 2^32)");
    const std::string err = check_sizes("mlmc_bootstrap_weights", sizes, nb, n);
    if (!err.empty()) return fail(err);
    BsScratch sc;
    struct Guard {
        BsScratch &s;
        ~Guard() { (void)wait_stream(rt().stream); bs_scratch_free(s); }
    } guard{sc};
    int64_t *d_sizes = nullptr;
    if (int rc = bs_scratch_alloc(sc)) return rc;
    const int64_t n_tiles = cdiv(n, BS_TILE);
    const int64_t rows = std::max<int64_t>(1, std::min<int64_t>({nb, (int64_t)65535, (int64_t)(BS_COUNTS_BYTES / 4) / n_tiles}));
    MLMC_HIP_CHECK(hipMalloc((void **)&d_sizes, sizeof(int64_t) * (size_t)nb));
    MLMC_HIP_CHECK(hipMemcpy(d_sizes, sizes, sizeof(int64_t) * (size_t)nb, hipMemcpyHostToDevice));
    int rc = 0;
    for (int64_t g = 0; g < nb && !rc; g += rows) {
        const int64_t ng = std::min(rows, nb - g);
        const int64_t mx = *std::max_element(sizes + g, sizes + g + ng);
        rc = launch_tile_counts(n, ng, d_sizes + g, mx, b0 + g, seed, stream, sc.counts);
        if (!rc) rc = launch_expand(n, ng, 0, n_tiles, sc.counts, b0 + g, seed, stream, w_out + g * n, n, 0);
    }
    hipError_t e = wait_stream(rt().stream);
    (void)hipFree(d_sizes);
    if (rc) return rc;
    if (e != hipSuccess) return fail(std::string("mlmc_bootstrap_weights: ") + hipGetErrorString(e));
    return 0;
}

extern "C" int mlmc_bootstrap_create(const mlmc_basis *b, int32_t M, int32_t n_levels, int64_t B, mlmc_bootstrap **out) {
    MLMC_API_GUARD;
    using namespace mlmc;
    const std::string e("mlmc_bootstrap_create");
    if (int rc = bs_create_check(e, n_levels, B)) return rc;
    if (!b || !out) return fail(e + ": null argument (basis, out)");
    if (b->p.kind != MLMC_LEGENDRE && b->p.kind != MLMC_MONOMIAL && b->p.kind != MLMC_FOURIER)
        return fail(e + ": basis kind " + std::to_string(b->p.kind) + " is not supported (Legendre, monomial and Fourier moments only)");
    if (b->out_size > 0) return fail(e + ": transformed bases are not supported");
    if (b->p.kind == MLMC_LEGENDRE && b->p.size > LEGENDRE_MAX_TERMS)
        return fail(e + ": Legendre size " + std::to_string(b->p.size) + " (at most " + std::to_string(LEGENDRE_MAX_TERMS) + ")");
    if (M < 1) return fail(e + ": M = " + std::to_string(M) + " (must be >= 1)");
    if ((int64_t)M * b->p.size > BS_MAX_COLS)
        return fail(e + ": M * R = " + std::to_string((int64_t)M * b->p.size) + " columns, at most " + std::to_string(BS_MAX_COLS) +
                    " are supported");
    mlmc_bootstrap *a = new mlmc_bootstrap();
    a->basis = b;
    a->M = M;
    a->L = n_levels;
    a->R = b->p.size;
    a->MR = M * b->p.size;
    a->B = B;
    a->keep_tiles = BS_TPR_MAX;
    const size_t tot = a->tot_bytes();
    if (hipMalloc((void **)&a->d_tot, tot) != hipSuccess || hipMalloc((void **)&a->d_cnt, sizeof(int64_t) * (size_t)n_levels * B) != hipSuccess ||
        bs_scratch_alloc(a->sc) != 0) {
        (void)hipGetLastError();
        mlmc_bootstrap_destroy(a);
        return fail(e + ": out of device memory (" + std::to_string(tot >> 20) + " MiB of totals + 64 MiB of scratch)");
    }
    MLMC_HIP_CHECK(hipMemsetAsync(a->d_tot, 0, tot, rt().stream));
    MLMC_HIP_CHECK(hipMemsetAsync(a->d_cnt, 0, sizeof(int64_t) * (size_t)n_levels * B, rt().stream));
    *out = a;
    return 0;
}

extern "C" void mlmc_bootstrap_destroy(mlmc_bootstrap *a) {
    if (!a) return;
    MLMC_API_GUARD;
    using namespace mlmc;
    (void)wait_stream(rt().stream);
    if (a->d_tot) (void)hipFree(a->d_tot);
    if (a->d_cnt) (void)hipFree(a->d_cnt);
    if (a->d_tab) (void)hipFree(a->d_tab);
    if (a->d_keep_m) (void)hipFree(a->d_keep_m);
    if (a->d_shift) (void)hipFree(a->d_shift);
    bs_scratch_free(a->sc);
    for (int64_t *p : a->h_sizes) (void)hipHostFree(p);
    for (hipEvent_t e : a->ev) (void)hipEventDestroy(e);
    delete a;
}

extern "C" int mlmc_bootstrap_reset(mlmc_bootstrap *a) {
    MLMC_API_GUARD;
    using namespace mlmc;
    if (!a) return fail("mlmc_bootstrap_reset: null handle");
    MLMC_HIP_CHECK(wait_stream(rt().stream));     // earlier chunks may still read the pinned sizes
    a->sizes_used = 0;
    a->ev_used = 0;
    MLMC_HIP_CHECK(hipMemsetAsync(a->d_tot, 0, a->tot_bytes(), rt().stream));
    if (a->d_cnt) MLMC_HIP_CHECK(hipMemsetAsync(a->d_cnt, 0, sizeof(int64_t) * (size_t)a->L * (size_t)a->B, rt().stream));
    if (a->xcov)            // the shift set since the previous reset takes effect now (mlmc_bootstrap_set_shift)
        MLMC_HIP_CHECK(hipMemcpyAsync(a->d_shift, a->shift_host.data(), sizeof(double) * a->shift_host.size(), hipMemcpyHostToDevice,
                                      rt().stream));
    a->pushes = 0;
    return 0;
}

extern "C" int mlmc_bootstrap_accum(mlmc_bootstrap *a, int32_t level, const double *fine, const double *coarse, int64_t n,
                                    const int64_t *sizes, uint64_t seed, uint32_t stream) {
    MLMC_API_GUARD;
    using namespace mlmc;
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (!a) return fail("mlmc_bootstrap_accum: null handle");
    if (!fine || !sizes) return fail("mlmc_bootstrap_accum: null argument (fine, sizes)");
    if (level < 0 || level >= a->L) return fail("mlmc_bootstrap_accum: level = " + std::to_string(level) + " (must be in 0 .. " + std::to_string(a->L - 1) + ")");
    if (n < 1 || n > BS_MAX_N)
        return fail("mlmc_bootstrap_accum: n = " + std::to_string(n) + " (must be in 1 .. " + std::to_string(BS_MAX_N) + ")");
    const std::string err = check_sizes("mlmc_bootstrap_accum", sizes, a->B, n);
    if (!err.empty()) return fail(err);
    const int64_t B = a->B;
    // the sizes go to a pinned block the kernels read in place: no copy to wait for, the block is reused after finalize / reset
    if (a->sizes_used == a->h_sizes.size()) {
        int64_t *p = nullptr;
        MLMC_HIP_CHECK(hipHostMalloc((void **)&p, sizeof(int64_t) * (size_t)B, hipHostMallocDefault));
        a->h_sizes.push_back(p);
    }
    int64_t *hs = a->h_sizes[a->sizes_used++];
    std::memcpy(hs, sizes, sizeof(int64_t) * (size_t)B);
    int64_t *ds = nullptr;
    MLMC_HIP_CHECK(hipHostGetDevicePointer((void **)&ds, hs, 0));
    a->pushes += 1;
    if (a->xcov) return bs_accum_xcov(a, level, fine, coarse, n, sizes, ds, seed, stream);
    return bs_accum(a, level, fine, coarse, n, sizes, ds, seed, stream);
}

extern "C" int mlmc_bootstrap_finalize(mlmc_bootstrap *a, int64_t *n_out, double *s_out, double *sp_out) {
    MLMC_API_GUARD;
    using namespace mlmc;
    if (!a) return fail("mlmc_bootstrap_finalize: null handle");
    if (a->multi) return fail("mlmc_bootstrap_finalize: the handle comes from mlmc_bootstrap_create_multi (use mlmc_bootstrap_finalize_multi)");
    if (a->xcov) return fail("mlmc_bootstrap_finalize: the handle comes from mlmc_bootstrap_create_xcov (use mlmc_bootstrap_finalize_xcov)");
    if (!n_out || !s_out || !sp_out) return fail("mlmc_bootstrap_finalize: null argument (n_out, s_out, sp_out)");
    const int64_t L = a->L, B = a->B, MR = a->MR;
    std::vector<double> tot((size_t)L * B * 2 * MR);
    std::vector<int64_t> cnt((size_t)L * B);
    MLMC_HIP_CHECK(hipMemcpyAsync(tot.data(), a->d_tot, sizeof(double) * tot.size(), hipMemcpyDeviceToHost, rt().stream));
    MLMC_HIP_CHECK(hipMemcpyAsync(cnt.data(), a->d_cnt, sizeof(int64_t) * cnt.size(), hipMemcpyDeviceToHost, rt().stream));
    MLMC_HIP_CHECK(wait_stream(rt().stream));
    a->sizes_used = 0;
    if (int rc = bs_time_collect(a)) return rc;
    const std::vector<double> &c = a->basis->scale_c;     // Legendre: P_r = c_r q_r of the scaled recurrence; else ones
    for (int64_t b = 0; b < B; ++b)
        for (int64_t l = 0; l < L; ++l) {
            n_out[b * L + l] = cnt[l * B + b];
            const double *t = tot.data() + (l * B + b) * 2 * MR;
            double *s = s_out + (b * L + l) * MR, *sp = sp_out + (b * L + l) * MR;
            for (int64_t j = 0; j < MR; ++j) {
                const double cj = c[j % a->R];
                s[j] = cj * t[j];
                sp[j] = (cj * cj) * t[MR + j];
            }
        }
    return 0;
}

extern "C" int mlmc_bootstrap_create_multi(int32_t M, const mlmc_basis *const *bases, int32_t K, int32_t n_levels, int64_t B,
                                           mlmc_bootstrap **out) {
    MLMC_API_GUARD;
    using namespace mlmc;
    const std::string e("mlmc_bootstrap_create_multi");
    if (int rc = bs_create_check(e, n_levels, B)) return rc;
    if (!bases || !out) return fail(e + ": null argument (bases, out)");
    if (M < 1 || M > 65535) return fail(e + ": M = " + std::to_string(M) + " (must be in 1 .. 65535)");
    if (K < 1 || K > 512) return fail(e + ": K must be in 1..512");
    std::vector<BasisParams> bps(M);
    for (int m = 0; m < M; ++m) {
        const mlmc_basis *b = bases[m];
        const std::string where = e + ": component " + std::to_string(m) + ": ";
        if (!b) return fail(where + "null basis");
        if (b->out_size > 0) return fail(where + "transformed bases are not supported (pass the family member of size K)");
        const int kind = b->p.kind;
        if (kind != MLMC_LEGENDRE && kind != MLMC_MONOMIAL && kind != MLMC_FOURIER)
            return fail(where + "only Legendre, monomial and Fourier moments");
        if (kind != bases[0]->p.kind) return fail(where + "every component must use the same family");
        if (b->p.size < K) return fail(where + "basis smaller than K");
        bps[m] = b->p;
    }
    // [n_levels][B][M (2 K + 1)] doubles; every factor is small enough for the product to stay inside 64 bits
    const uint64_t tot_elems = (uint64_t)n_levels * (uint64_t)B * (uint64_t)M * (uint64_t)(2 * K + 1);
    if (tot_elems > ((uint64_t)2 << 30) / sizeof(double))
        return fail(e + ": the totals [n_levels][B][M (2 K + 1)] = [" + std::to_string(n_levels) + "][" + std::to_string(B) + "][" +
                    std::to_string((int64_t)M * (2 * K + 1)) + "] doubles take " + std::to_string((tot_elems * sizeof(double)) >> 20) +
                    " MiB, at most 2048 MiB are supported (fewer replicates or components per call)");
    mlmc_bootstrap *a = new mlmc_bootstrap();
    a->multi = true;
    a->basis = bases[0];
    a->bases.assign(bases, bases + M);
    a->M = M;
    a->L = n_levels;
    a->R = K;
    a->MR = M * K;
    a->B = B;
    // keep bytes [M][range]: the range shrinks with M so that they stay within 8 MiB (one tile at least)
    a->keep_tiles = std::max<int64_t>(1, std::min<int64_t>(BS_TPR_MAX, (int64_t)((size_t)8 << 20) / ((int64_t)M * BS_TILE)));
    const size_t tot = a->tot_bytes();
    if (hipMalloc((void **)&a->d_tot, tot) != hipSuccess || hipMalloc((void **)&a->d_tab, sizeof(BasisParams) * (size_t)M) != hipSuccess ||
        hipMalloc((void **)&a->d_keep_m, (size_t)M * a->keep_tiles * BS_TILE) != hipSuccess || bs_scratch_alloc(a->sc) != 0) {
        (void)hipGetLastError();
        mlmc_bootstrap_destroy(a);
        return fail(e + ": out of device memory (" + std::to_string(tot >> 20) + " MiB of totals + 64 MiB of scratch + keep bytes)");
    }
    hipError_t err = hipMemcpy(a->d_tab, bps.data(), sizeof(BasisParams) * (size_t)M, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemsetAsync(a->d_tot, 0, tot, rt().stream);
    if (err != hipSuccess) {
        mlmc_bootstrap_destroy(a);
        return fail(e + ": " + hipGetErrorString(err));
    }
    *out = a;
    return 0;
}

extern "C" int mlmc_bootstrap_finalize_multi(mlmc_bootstrap *a, int64_t *n_out, double *s_out, double *sp_out) {
    MLMC_API_GUARD;
    using namespace mlmc;
    if (!a) return fail("mlmc_bootstrap_finalize_multi: null handle");
    if (a->xcov) return fail("mlmc_bootstrap_finalize_multi: the handle comes from mlmc_bootstrap_create_xcov (use mlmc_bootstrap_finalize_xcov)");
    if (!a->multi) return fail("mlmc_bootstrap_finalize_multi: the handle comes from mlmc_bootstrap_create (use mlmc_bootstrap_finalize)");
    if (!n_out || !s_out || !sp_out) return fail("mlmc_bootstrap_finalize_multi: null argument (n_out, s_out, sp_out)");
    const int64_t L = a->L, B = a->B, M = a->M, K = a->R, C = 2 * K + 1;
    std::vector<double> tot((size_t)L * B * M * C);
    MLMC_HIP_CHECK(hipMemcpyAsync(tot.data(), a->d_tot, sizeof(double) * tot.size(), hipMemcpyDeviceToHost, rt().stream));
    MLMC_HIP_CHECK(wait_stream(rt().stream));
    a->sizes_used = 0;
    if (int rc = bs_time_collect(a)) return rc;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t l = 0; l < L; ++l)
            for (int64_t m = 0; m < M; ++m) {
                const double *t = tot.data() + ((l * B + b) * M + m) * C;
                const std::vector<double> &c = a->bases[m]->scale_c;     // Legendre: P_k = c_k q_k; else ones
                const int64_t o = (b * L + l) * M + m;
                n_out[o] = (int64_t)t[2 * K];                            // an exact integer (BsPerComponent)     
                for (int64_t k = 0; k < K; ++k) {
                    s_out[o * K + k] = c[k] * t[k];
                    sp_out[o * K + k] = (c[k] * c[k]) * t[K + k];
                }
            }
    return 0;
}

extern "C" int mlmc_bootstrap_create_xcov(int32_t M, int32_t n_levels, int64_t B, mlmc_bootstrap **out) {
    MLMC_API_GUARD;
    using namespace mlmc;
    const std::string e("mlmc_bootstrap_create_xcov");
    if (int rc = bs_create_check(e, n_levels, B)) return rc;
    if (!out) return fail(e + ": null argument (out)");
    if (M < 1 || M > BSX_MAX_M) return fail(e + ": M = " + std::to_string(M) + " (must be in 1 .. " + std::to_string(BSX_MAX_M) + ")");
    const int64_t C = bsx_cols(M);
    // [n_levels][B][C] doubles; every factor is small enough for the product to stay inside 64 bits
    const uint64_t tot_elems = (uint64_t)n_levels * (uint64_t)B * (uint64_t)C;
    if (tot_elems > ((uint64_t)2 << 30) / sizeof(double))
        return fail(e + ": the totals [n_levels][B][1 + M + M (M + 1) / 2] = [" + std::to_string(n_levels) + "][" + std::to_string(B) + "][" +
                    std::to_string(C) + "] doubles take " + std::to_string((tot_elems * sizeof(double)) >> 20) +
                    " MiB, at most 2048 MiB are supported (fewer replicates or components per call)");
    mlmc_bootstrap *a = new mlmc_bootstrap();
    a->xcov = true;
    a->M = M;
    a->L = n_levels;
    a->B = B;
    a->C = C;
    a->keep_tiles = BS_TPR_MAX;
    a->shift_host.assign(M, 0.0);
    const size_t tot = a->tot_bytes();
    if (hipMalloc((void **)&a->d_tot, tot) != hipSuccess || hipMalloc((void **)&a->d_shift, sizeof(double) * (size_t)M) != hipSuccess ||
        bs_scratch_alloc(a->sc) != 0) {
        (void)hipGetLastError();
        mlmc_bootstrap_destroy(a);
        return fail(e + ": out of device memory (" + std::to_string(tot >> 20) + " MiB of totals + 64 MiB of scratch)");
    }
    hipError_t err = hipMemsetAsync(a->d_tot, 0, tot, rt().stream);
    if (err == hipSuccess) err = hipMemsetAsync(a->d_shift, 0, sizeof(double) * (size_t)M, rt().stream);
    if (err != hipSuccess) {
        mlmc_bootstrap_destroy(a);
        return fail(e + ": " + hipGetErrorString(err));
    }
    *out = a;
    return 0;
}

extern "C" int mlmc_bootstrap_set_shift(mlmc_bootstrap *a, const double *shift_host) {
    MLMC_API_GUARD;
    using namespace mlmc;
    if (!a) return fail("mlmc_bootstrap_set_shift: null argument");
    if (!a->xcov) return fail("mlmc_bootstrap_set_shift: not a component-covariance handle (mlmc_bootstrap_create_xcov)");
    if (a->pushes > 0) return fail("mlmc_bootstrap_set_shift: pushes are pending; reset the accumulator first");
    if (shift_host)
        for (int m = 0; m < a->M; ++m)
            if (!std::isfinite(shift_host[m])) return fail("mlmc_bootstrap_set_shift: shift[" + std::to_string(m) + "] is not finite");
    MLMC_HIP_CHECK(wait_stream(rt().stream));    // the previous reset's upload reads shift_host
    if (shift_host) std::memcpy(a->shift_host.data(), shift_host, sizeof(double) * (size_t)a->M);
    else std::fill(a->shift_host.begin(), a->shift_host.end(), 0.0);
    return 0;
}

extern "C" int mlmc_bootstrap_finalize_xcov(mlmc_bootstrap *a, int64_t *n_out, double *s1_out, double *s2_out) {
    MLMC_API_GUARD;
    using namespace mlmc;
    if (!a) return fail("mlmc_bootstrap_finalize_xcov: null handle");
    if (!a->xcov)
        return fail(std::string("mlmc_bootstrap_finalize_xcov: the handle comes from ") +
                    (a->multi ? "mlmc_bootstrap_create_multi (use mlmc_bootstrap_finalize_multi)" : "mlmc_bootstrap_create (use mlmc_bootstrap_finalize)"));
    if (!n_out || !s1_out || !s2_out) return fail("mlmc_bootstrap_finalize_xcov: null argument (n_out, s1_out, s2_out)");
    const int64_t L = a->L, B = a->B, M = a->M, C = a->C;
    std::vector<double> tot((size_t)L * B * C);
    MLMC_HIP_CHECK(hipMemcpyAsync(tot.data(), a->d_tot, sizeof(double) * tot.size(), hipMemcpyDeviceToHost, rt().stream));
    MLMC_HIP_CHECK(wait_stream(rt().stream));
    a->sizes_used = 0;
    if (int rc = bs_time_collect(a)) return rc;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t l = 0; l < L; ++l) {
            const double *t = tot.data() + (l * B + b) * C;
            const int64_t o = b * L + l;
            n_out[o] = (int64_t)t[0];                                     // an exact integer (the flag column)
            std::memcpy(s1_out + o * M, t + 1, sizeof(double) * (size_t)M);
            double *s2 = s2_out + o * M * M;
            const double *q = t + 1 + M;
            for (int64_t i = 0; i < M; ++i)
                for (int64_t j = i; j < M; ++j) {
                    const double v = *q++;                                // one computed value goes to (i, j) and (j, i)
                    s2[i * M + j] = v;
                    s2[j * M + i] = v;
                }
        }
    return 0;
}

extern "C" int mlmc_bootstrap_kernel_time(mlmc_bootstrap *a, double *ms_contract, double *ms_rng, int64_t *mfma_flops) {
    MLMC_API_GUARD;
    using namespace mlmc;
    if (!a) return fail("mlmc_bootstrap_kernel_time: null handle");
    MLMC_HIP_CHECK(wait_stream(rt().stream));
    if (int rc = bs_time_collect(a)) return rc;
    if (ms_contract) *ms_contract = a->ms_contract;
    if (ms_rng) *ms_rng = a->ms_rng;
    if (mfma_flops) *mfma_flops = a->flops;
    a->ms_contract = a->ms_rng = 0;
    a->flops = 0;
    return 0;
}
