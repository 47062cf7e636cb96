// mlmc_concordance_counts (include/mlmc_hip.h): how often the components of a vector lie inside a box event -- pair by pair, all at
// once, fine against coarse -- counted on bits (gfx950).  Everything is integer: no result depends on the launch geometry.
//
//   k_conc_bits : streams the values ONCE.  A wave owns 64 consecutive columns (one word) at a time, a lane one column: per component
//                 two coalesced 512-byte loads (fine, coarse), the NaN ballot, and per event the ballots of lower < v && v < upper.
//                 The limits are wave-uniform (scalar loads).  Lane g * S + s keeps the word of (event g, side s) of the row and the
//                 lanes below G * S store them to bits[g][s][m][w] (S = 2 with a coarse array, else 1); lane g / 16 + g carries
//                 the AND over the rows of the fine / coarse words of event g.  The keep word -- the columns below n without a NaN
//                 in any row -- is known only after the last row, so it is not ANDed into the stored words here (that would take a
//                 second pass over the values or the words): it goes to keep[w] and k_conc_gram applies it when it stages a word,
//                 one AND per staged word.  The counts of A^f, A^c, A^f != A^c and of the kept columns stay in a lane register over
//                 the words of a wave (a grid-stride loop), the four waves add up in LDS and the block stores 64 partial counts.
//   k_conc_all  : one workgroup adds the blocks' partials and adds the sums to the caller's `all` and `kept` (plain adds: one
//                 stream; integers, so the order of the partials is free).
//   k_conc_gram : the binary Gram.  A workgroup owns a 32 x 32 tile of pairs (a, b) of tile rows ta <= tb, one event and a run of
//                 words; it stages 32 words of its 2 x 32 rows (fine and coarse) in LDS as [row][33] -- the odd pitch keeps the 16
//                 rows that the lanes of a half wave read at once on different banks of the 8-byte reads -- ANDed with keep, and a
//                 thread counts popcount(a & b) of its 2 x 2 pairs in 32-bit registers: J^f, J^c and J^f ^ J^c.  A run is at most
//                 2^20 words (2^26 columns), so a count stays below 2^31.  One atomicAdd per (statistic, pair) and workgroup into
//                 the int64 counters, and the same into the mirrored entry (b, a): integer adds commute, so the order is free.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"

namespace mlmc {

constexpr int CC_THREADS = 256;
constexpr int CC_WAVES = CC_THREADS / WAVE;
constexpr int CC_ROWS = 4;                            // rows whose loads are in flight together
constexpr int CA_THREADS = 1024;                      // k_conc_all
constexpr int CA_WAVES = CA_THREADS / WAVE;
constexpr int CC_PART = 64;                           // partial counts of a block: lane k * 16 + g (k = 0 f, 1 c, 2 x), lane 63 kept
constexpr int CG_TILE = 32;                           // pair tile of k_conc_gram
constexpr int CG_WORDS = 32;                          // words staged at once
constexpr int CG_PITCH = CG_WORDS + 1;
constexpr int64_t CG_MAX_RUN = (int64_t)1 << 20;      // words of a run: 64 * 2^20 < 2^31
constexpr size_t CC_BITS_BYTES = (size_t)256 << 20;   // the bit matrix of one slab of columns

template <bool COARSE, bool BITS, bool ALL>
__global__ __launch_bounds__(CC_THREADS) void k_conc_bits(const double *__restrict__ fine, const double *__restrict__ coarse, int M,
                                                          int64_t n, int64_t ld, int G, const double *__restrict__ lo,
                                                          const double *__restrict__ hi, int64_t W, uint64_t *__restrict__ bits,
                                                          uint64_t *__restrict__ keep_out, int64_t *__restrict__ part) {
    constexpr int S = COARSE ? 2 : 1;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * CC_WAVES;
    const double nan = __builtin_nan("");
    int64_t cnt = 0;
    for (int64_t w = (int64_t)blockIdx.x * CC_WAVES + wave; w < W; w += n_waves) {      // wave-uniform
        const int64_t j = w * WAVE + lane;
        const bool valid = j < n;                      // the tail of the last word: masked by the column count
        const uint64_t tail = __ballot(valid);
        uint64_t nanw = 0, acc = ~(uint64_t)0;
        const auto row = [&](int m, double f, double c) {
            nanw |= __ballot(f != f);
            if (COARSE) nanw |= __ballot(c != c);
            uint64_t mine = 0;
            for (int g = 0; g < G; ++g) {
                const double l = lo[(int64_t)g * M + m], h = hi[(int64_t)g * M + m];
                const uint64_t wf = __ballot(l < f && f < h);
                if (ALL) acc = lane == g ? acc & wf : acc;
                if (BITS) mine = lane == g * S ? wf : mine;
                if (COARSE) {
                    const uint64_t wc = __ballot(l < c && c < h);
                    if (ALL) acc = lane == 16 + g ? acc & wc : acc;
                    if (BITS) mine = lane == g * S + 1 ? wc : mine;
                }
            }
            if (BITS && lane < G * S) bits[((int64_t)lane * M + m) * W + w] = mine;      // lane = g * S + s
        };
        // CC_ROWS rows at a time: their loads are issued together, then the rows are worked off in order
        for (int m0 = 0; m0 < M; m0 += CC_ROWS) {
            double f[CC_ROWS], c[CC_ROWS];
#pragma unroll
            for (int u = 0; u < CC_ROWS; ++u) {
                const int64_t at = (int64_t)std::min(m0 + u, M - 1) * ld + j;            // beyond M: the last row again, not used
                f[u] = valid ? fine[at] : nan;
                c[u] = COARSE ? (valid ? coarse[at] : nan) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < CC_ROWS; ++u)
                if (m0 + u < M) row(m0 + u, f[u], c[u]);
        }
        const uint64_t keep = tail & ~nanw;
        if (BITS && lane == 0) keep_out[w] = keep;
        uint64_t af = 0, ac = 0;
        if (ALL) {
            af = __shfl(acc, lane & 15) & keep;
            if (COARSE) ac = __shfl(acc, 16 + (lane & 15)) & keep;
        }
        const int k = lane >> 4;
        const uint64_t v = k == 0 ? af : k == 1 ? ac : k == 2 ? af ^ ac : keep;
        cnt += __popcll(v);                            // lanes k * 16 + g with g >= G: not read
    }
    __shared__ int64_t red[CC_WAVES][WAVE];
    red[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0) part[(int64_t)blockIdx.x * CC_PART + lane] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// one workgroup: wave v adds the blocks v, v + CA_WAVES, ... (eight loads in flight), the waves add up in LDS in order
__global__ __launch_bounds__(CA_THREADS) void k_conc_all(const int64_t *__restrict__ part, int n_blocks, int G, int64_t *__restrict__ all,
                                                         int64_t *__restrict__ kept) {
    __shared__ int64_t red[CA_WAVES][WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    int64_t s = 0;
#pragma unroll 8
    for (int b = wave; b < n_blocks; b += CA_WAVES) s += part[(int64_t)b * CC_PART + lane];
    red[wave][lane] = s;
    __syncthreads();
    if (wave) return;
    s = 0;
#pragma unroll
    for (int v = 0; v < CA_WAVES; ++v) s += red[v][lane];
    const int k = lane >> 4, g = lane & 15;
    if (all && k < 3 && g < G) all[g * 3 + k] += s;
    if (kept && lane == WAVE - 1) kept[0] += s;
}

__device__ __forceinline__ void conc_add(int64_t *p, int v) {
    if (v) atomicAdd((unsigned long long *)p, (unsigned long long)v);
}

// grid (tile pairs ta <= tb, events, runs)
template <bool COARSE>
__global__ __launch_bounds__(CC_THREADS) void k_conc_gram(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ keep, int M,
                                                          int64_t W, int64_t run, int n_tiles, int64_t *__restrict__ pair) {
    constexpr int S = COARSE ? 2 : 1;
    __shared__ uint64_t sa[S][CG_TILE][CG_PITCH], sb[S][CG_TILE][CG_PITCH];
    int t = blockIdx.x, ta = 0;
    while (t >= n_tiles - ta) {
        t -= n_tiles - ta;
        ++ta;
    }
    const int tb = ta + t, g = blockIdx.y;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int a0 = ta * CG_TILE + 2 * ty, b0 = tb * CG_TILE + 2 * tx;
    const bool live = a0 < M && b0 < M && b0 + 1 >= a0;           // some pair a <= b of the thread exists
    int cf[2][2] = {{0, 0}, {0, 0}}, cc[2][2] = {{0, 0}, {0, 0}}, cx[2][2] = {{0, 0}, {0, 0}};
    const int64_t w_begin = (int64_t)blockIdx.z * run, w_end = std::min<int64_t>(W, w_begin + run);
    for (int64_t w0 = w_begin; w0 < w_end; w0 += CG_WORDS) {
        const int nw = (int)std::min<int64_t>(CG_WORDS, w_end - w0);
        __syncthreads();
        for (int idx = threadIdx.x; idx < S * CG_TILE * CG_WORDS; idx += CC_THREADS) {
            const int wi = idx % CG_WORDS, r = idx / CG_WORDS % CG_TILE, s = idx / (CG_WORDS * CG_TILE);
            const int ma = ta * CG_TILE + r, mb = tb * CG_TILE + r;
            const bool in = wi < nw;
            const uint64_t kw = in ? keep[w0 + wi] : 0;                                  // rows beyond M and words beyond the run: 0
            const int64_t row = (int64_t)(g * S + s) * M;
            sa[s][r][wi] = in && ma < M ? bits[(row + ma) * W + w0 + wi] & kw : 0;
            sb[s][r][wi] = in && mb < M ? bits[(row + mb) * W + w0 + wi] & kw : 0;
        }
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (int wi = 0; wi < CG_WORDS; ++wi) {
                uint64_t af[2], bf[2], ac[2], bc[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    af[i] = sa[0][2 * ty + i][wi];
                    bf[i] = sb[0][2 * tx + i][wi];
                    if (COARSE) {
                        ac[i] = sa[S - 1][2 * ty + i][wi];
                        bc[i] = sb[S - 1][2 * tx + i][wi];
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const uint64_t jf = af[i] & bf[k];
                        cf[i][k] += __popcll(jf);
                        if (COARSE) {
                            const uint64_t jc = ac[i] & bc[k];
                            cc[i][k] += __popcll(jc);
                            cx[i][k] += __popcll(jf ^ jc);
                        }
                    }
            }
        }
    }
    if (!live) return;
    const int64_t MM = (int64_t)M * M;
    int64_t *pg = pair + (int64_t)g * 3 * MM;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int a = a0 + i, b = b0 + k;
            if (a >= M || b >= M || a > b) continue;
            // without a coarse array J^c = 0: the two joint indicators differ where J^f = 1
            const int v[3] = {cf[i][k], COARSE ? cc[i][k] : 0, COARSE ? cx[i][k] : cf[i][k]};
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                conc_add(pg + q * MM + (int64_t)a * M + b, v[q]);
                if (a != b) conc_add(pg + q * MM + (int64_t)b * M + a, v[q]);
            }
        }
}

template <bool COARSE>
static void launch_conc_bits(bool with_bits, bool with_all, int blocks, hipStream_t st, const double *fine, const double *coarse, int M,
                             int64_t n, int64_t ld, int G, const double *lo, const double *hi, int64_t W, uint64_t *bits, uint64_t *keep,
                             int64_t *part) {
    const dim3 grid((unsigned)blocks), block(CC_THREADS);
    if (with_bits && with_all)
        hipLaunchKernelGGL((k_conc_bits<COARSE, true, true>), grid, block, 0, st, fine, coarse, M, n, ld, G, lo, hi, W, bits, keep, part);
    else if (with_bits)
        hipLaunchKernelGGL((k_conc_bits<COARSE, true, false>), grid, block, 0, st, fine, coarse, M, n, ld, G, lo, hi, W, bits, keep, part);
    else
        hipLaunchKernelGGL((k_conc_bits<COARSE, false, true>), grid, block, 0, st, fine, coarse, M, n, ld, G, lo, hi, W, bits, keep, part);
}

// event pairs around the two kernels of a call that asks for their time (kernel_ms); best effort, like the other timings
struct ConcTiming {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ok = false;
    bool ready() {
        if (!ok) {
            ok = true;
            for (auto &e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
        }
        return ok;
    }
};

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_concordance_counts(const double *fine, const double *coarse, int32_t M, int64_t n, int64_t ld, int32_t G, const double *lower,
                            const double *upper, int64_t *pair, int64_t *all, int64_t *kept, double *kernel_ms) {
    MLMC_API_GUARD;
    const std::string e("mlmc_concordance_counts");
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (M < 0 || n < 0 || G < 1)
        return fail(e + ": M = " + std::to_string(M) + ", n = " + std::to_string(n) + ", G = " + std::to_string(G) +
                    " (M, n >= 0 and G >= 1 are required)");
    if (M > MLMC_CONCORDANCE_MAX_M)
        return fail(e + ": M = " + std::to_string(M) + " is above the cap " + std::to_string(MLMC_CONCORDANCE_MAX_M));
    if (G > MLMC_CONCORDANCE_MAX_G)
        return fail(e + ": G = " + std::to_string(G) + " is above the cap " + std::to_string(MLMC_CONCORDANCE_MAX_G));
    if (ld < n) return fail(e + ": row stride ld = " + std::to_string(ld) + " is below n = " + std::to_string(n));
    if (!lower || !upper) return fail(e + ": null limits");
    if (!pair && !all) return fail(e + ": both counter arrays are null");
    for (int64_t i = 0; i < (int64_t)G * M; ++i)
        if (lower[i] != lower[i] || upper[i] != upper[i])
            return fail(e + ": a limit of event " + std::to_string(i / M) + ", component " + std::to_string(i % M) + " is NaN");
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0;
    if (M == 0 || n == 0) return 0;
    if (!fine) return fail(e + ": null fine");

    hipStream_t st = rt().stream;
    const int S = coarse ? 2 : 1;
    // a slab of columns: whole staging groups of words whose bit matrix [G][S][M][words] stays within CC_BITS_BYTES
    const int64_t W_all = (n + WAVE - 1) / WAVE;
    int64_t slab = (int64_t)(CC_BITS_BYTES / (sizeof(uint64_t) * (size_t)G * S * M)) / CG_WORDS * CG_WORDS;
    slab = std::max<int64_t>(slab, CG_WORDS);
    if (!pair) slab = W_all;                                          // no bit matrix
    // MLMC_CONCORDANCE_SLAB_WORDS in the environment, read per call, sets the words of a slab, rounded up to whole staging groups
    // (a test aid: the counters are integers, no value depends on it)
    if (const char *env = std::getenv("MLMC_CONCORDANCE_SLAB_WORDS")) {
        const long long v = std::atoll(env);
        if (v > 0) slab = std::min<int64_t>(slab, (v + CG_WORDS - 1) / CG_WORDS * CG_WORDS);
    }
    slab = std::min(slab, W_all);
    const int max_blocks = 8 * std::max(rt().n_cu, 1);
    const int blocks_cap = (int)std::min<int64_t>((slab + CC_WAVES - 1) / CC_WAVES, max_blocks);
    const size_t b_lim = mm_align(sizeof(double) * 2 * (size_t)G * M), b_part = mm_align(sizeof(int64_t) * CC_PART * (size_t)blocks_cap);
    const size_t b_keep = pair ? mm_align(sizeof(uint64_t) * (size_t)slab) : 0;
    const size_t b_bits = pair ? mm_align(sizeof(uint64_t) * (size_t)G * S * M * (size_t)slab) : 0;
    static MultiWorkspace ws;
    if (ws.reserve(b_lim + b_part + b_keep + b_bits)) return 1;
    double *d_lo = (double *)ws.dev, *d_hi = d_lo + (size_t)G * M;
    int64_t *d_part = (int64_t *)(ws.dev + b_lim);
    uint64_t *d_keep = (uint64_t *)(ws.dev + b_lim + b_part), *d_bits = (uint64_t *)(ws.dev + b_lim + b_part + b_keep);
    std::vector<double> lim(2 * (size_t)G * M);
    std::memcpy(lim.data(), lower, sizeof(double) * (size_t)G * M);
    std::memcpy(lim.data() + (size_t)G * M, upper, sizeof(double) * (size_t)G * M);
    MLMC_HIP_CHECK(hipMemcpyAsync(d_lo, lim.data(), sizeof(double) * lim.size(), hipMemcpyHostToDevice, st));

    static ConcTiming tm;
    const int n_tiles = (M + CG_TILE - 1) / CG_TILE, tile_pairs = n_tiles * (n_tiles + 1) / 2;
    int64_t n_slabs = 0;
    for (int64_t w0 = 0; w0 < W_all; w0 += slab, ++n_slabs) {
        const int64_t W = std::min(slab, W_all - w0), c0 = w0 * WAVE, nc = std::min<int64_t>(n - c0, W * WAVE);
        const int blocks = (int)std::min<int64_t>((W + CC_WAVES - 1) / CC_WAVES, max_blocks);
        const bool timed = kernel_ms && n_slabs == 0 && tm.ready();   // the first slab of the call
        if (timed) (void)hipEventRecord(tm.ev[0], st);
        if (coarse)
            launch_conc_bits<true>(pair, all, blocks, st, fine + c0, coarse + c0, M, nc, ld, G, d_lo, d_hi, W, d_bits, d_keep, d_part);
        else
            launch_conc_bits<false>(pair, all, blocks, st, fine + c0, nullptr, M, nc, ld, G, d_lo, d_hi, W, d_bits, d_keep, d_part);
        if (timed) (void)hipEventRecord(tm.ev[1], st);
        if (all || kept) hipLaunchKernelGGL(k_conc_all, dim3(1), dim3(CA_THREADS), 0, st, (const int64_t *)d_part, blocks, (int)G, all, kept);
        if (pair) {
            // runs: enough workgroups to fill the device, whole staging groups, counts below 2^31
            const int64_t want = std::max<int64_t>(1, (4 * (int64_t)std::max(rt().n_cu, 1)) / ((int64_t)tile_pairs * G));
            int64_t run = (W + want - 1) / want;
            run = std::min((run + CG_WORDS - 1) / CG_WORDS * CG_WORDS, CG_MAX_RUN);
            const dim3 grid((unsigned)tile_pairs, (unsigned)G, (unsigned)((W + run - 1) / run));
            if (timed) (void)hipEventRecord(tm.ev[2], st);
            if (coarse)
                hipLaunchKernelGGL(k_conc_gram<true>, grid, dim3(CC_THREADS), 0, st, (const uint64_t *)d_bits, (const uint64_t *)d_keep,
                                   (int)M, W, run, n_tiles, pair);
            else
                hipLaunchKernelGGL(k_conc_gram<false>, grid, dim3(CC_THREADS), 0, st, (const uint64_t *)d_bits, (const uint64_t *)d_keep,
                                   (int)M, W, run, n_tiles, pair);
            if (timed) (void)hipEventRecord(tm.ev[3], st);
        }
        MLMC_HIP_CHECK(hipGetLastError());
    }
    MLMC_HIP_CHECK(wait_stream(st));
    if (kernel_ms && tm.ok) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, tm.ev[0], tm.ev[1]) == hipSuccess) kernel_ms[0] = ms;
        if (pair && hipEventElapsedTime(&ms, tm.ev[2], tm.ev[3]) == hipSuccess) kernel_ms[1] = ms;
    }
    return 0;
}

}  // extern "C"
