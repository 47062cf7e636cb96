// mlmc_copula_box_prob_batch (include/mlmc_hip.h): rectangle probabilities of a correlated normal vector by Genz's separation of
// variables, on the device (gfx950).
//
//   k_box_prob : one workgroup of ONE wave owns the 64 points j = 64 a .. 64 a + 63 (a = an absolute block of the sequence) of one
//                (seed, box); a lane owns one point and runs the M-step chain of the header: two normcdf, one normcdfinv and the
//                triangular dot product of step i.  The lane's y_0 .. y_{M-2} live in LDS as y[k][lane] (dynamic, 512 (M - 1) bytes
//                per workgroup: small M keeps its occupancy, the cap M = 128 takes 65024 bytes); a lane reads back only what it
//                wrote itself, so the chain needs no barrier.  L, the limits and the shift are uniform over the wave: the compiler
//                fetches them with scalar loads.  Under MLMC_SAMPLE_SOBOL the block is aligned to 64 points, so the Gray code of
//                j = 64 a ^ lane is G(64 a) ^ G(lane): the part of the block is an XOR of scalar loads, the lane adds at most six
//                of the words V'[0 .. 5].  The wave sums its 64 values in a fixed butterfly and lane 0 stores the block's partial.
//                The DRAWS instances (mlmc_copula_box_draws_batch) are the same text: they also take a coordinate for the last
//                component, keep its y in a register, and store every step's score z_i (clamped to its limits) and, if asked,
//                its normcdf at column j of row (seed, box, i): a wave writes 64 consecutive doubles per component.
//                The TCOP instances (mlmc_copula_box_prob_t_batch / _draws_t_batch: the Student-t copula by Genz and Bretz's mixing
//                variable) are again the same text: a lane reads its point's mixing scale, which k_box_mixing (copula_t.hip) has
//                made once per (seed, point) before the launch, divides every limit by it and scales the stored score; the t CDF
//                of the draws is a pass of k_tcop_map over the rows of scores afterwards.  Neither chi2_mixing_scale nor
//                student_t_cdf is called from the chain: their series loops and constants stay out of the loop over i
//                (DESIGN.md 3.5.23).
//                The TCOND instances (mlmc_copula_box_prob_tc_batch / _draws_tc_batch: a CONDITIONAL law of the t copula, location
//                shift[b], scale matrix scale[b]^2 L L^T, the mixing variable with dof_mix degrees of freedom) are TCOP with one more
//                flag: the lane multiplies its mixing scale by the box's scale once, takes the shift off every limit before the
//                division, and adds it back to the stored t score.
//                The LEAD instances (mlmc_copula_box_prob_tl_batch / _draws_tl_batch: the t copula with component 0 drawn INSIDE its
//                limits and the mixing scale conditioned on it) are TCOP with one more flag: k_box_lead
//                (copula_t.hip) has made the lead score v and the scale sc per (seed, box, point); the chain starts at i = 1 with
//                y_0 = v / sc and the finished product of widths is multiplied by the lead's weight W0 of the box.  Again no t
//                function is called from the chain.
//                The _pf_ entries (one factor PER BOX, for Genz's variable reordering of box_order.hip and for bootstrap replicates) are
//                the same instances: the kernel adds b * fstride to L, fstride = 0 for every other entry.  b is blockIdx.y, so the
//                factor stays uniform over the wave and on the scalar unit; no operation of a point knows whether its factor is shared.
//   k_box_mean : one workgroup per (seed, box) sums the partials of its blocks in a fixed tree and divides by n.
// The tree: lanes outside [first, first + n) add +0; the wave adds v += v(lane ^ 32), ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; thread t of
// k_box_mean adds the partials t, t + 256, ... in ascending order from 0 and the 256 sums fold by halves (128, 64, ... 1).  It is
// fixed by (first, n) alone.  Launches are split by whole blocks, so no value depends on the split.
// The chain loops over i around normcdf / normcdfinv; copula.hip and sobol.hip avoid such a loop because the inlined functions'
// constants then stay in registers.  Here the two are called through functions that are not inlined (below); the resource figures
// are in DESIGN.md 3.5.17 and 3.5.18.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "copula.hpp"
#include "sobol.hpp"

namespace mlmc {

constexpr int BOX_LANES = 64;                          // points of a block = lanes of its wave
constexpr int BOX_MEAN_THREADS = 256;
constexpr size_t BOX_F_BYTES = (size_t)192 << 20;      // the staged integrand of a launch (host f_out)
constexpr size_t BOX_PARTIAL_BYTES = (size_t)1 << 30;  // the partials of a call

// coordinate of point j = 64 a ^ lane from its dimension's row: the block's part on the scalar unit, the lane's six bits selected
__device__ __forceinline__ double box_sobol_unit(const uint64_t *__restrict__ row, uint64_t a, int lane) {
    const uint64_t j0 = a << 6;
    uint64_t g = j0 ^ (j0 >> 1), m = row[SOBOL_BITS];
    while (g) {
        m ^= row[__builtin_ctzll(g)];                  // bit 52 only for the lanes beyond the last point of a call that ends at 2^52
        g &= g - 1;
    }
    const uint32_t gl = (uint32_t)lane ^ ((uint32_t)lane >> 1);
#pragma unroll
    for (int t = 0; t < 6; ++t) m ^= ((gl >> t) & 1u) ? row[t] : (uint64_t)0;
    return sobol_unit(m);
}

// Called, not inlined: inlined into the loop over i their constants stay in registers across it (256 VGPRs, 156 AGPRs and scratch
// instead of 30 / 38 VGPRs and none); a call costs a few cycles next to the hundred-odd fp64 operations of a body.
__device__ __attribute__((noinline)) double box_normcdf(double x) { return normcdf(x); }
__device__ __attribute__((noinline)) double box_normcdfinv(double p) { return normcdfinv(p); }

// grid (blocks of the launch, boxes, seeds); box = b0 + blockIdx.y, seed = r0 + blockIdx.z.  DRAWS (mlmc_copula_box_draws_batch): the
// same chain, one text; coordinate M - 1 draws the last component too (its y stays in a register), and every step stores the
// score z_i = s + L_ii y_i clamped to its limits, and its normcdf, at column j of row i: consecutive lanes, consecutive doubles.
// TCOP (the t entries): `mix` holds the mixing scales of the launch, sc = mix[seed][64 blockIdx.x + lane] (k_box_mixing; a block
// of gridDim.x * 64 doubles per seed of the call).  Every limit is divided by sc, the chain runs on the quotients without a shift, the
// stored score is the t score min(max(z sc, l), h), and a row of u_out receives the same score: the CDF pass maps it in place.
// TCOND (the tc entries, with TCOP): sc = scl[b] * sc once (scl NULL: ones); with a shift every limit is (lo - shift) / sc, one
// rounded subtraction before the division, the chain itself runs without a shift, and the stored score is
// min(max(shift + z sc, lo), hi).  With shift NULL neither the subtraction nor the sum is taken: the bits of TCOP.
// LEAD (the tl entries, with TCOP and without TCOND): the three pointers that a t entry leaves unused carry the lead's arrays, so that
// every other instance keeps its arguments: `shift` holds W0 [B], `mix` holds sc and `scl` holds v, both
// [seed][box][64 blockIdx.x + lane] over the R * B pairs of the call (k_box_lead).  ys[0] = v / sc, one division; steps 1 .. M - 1
// are TCOP's; f = W0 * (the product of their widths), one rounded product at the end; with DRAWS row 0 is min(max(v L_00, lo), hi).
template <bool SOBOL, bool DRAWS, bool TCOP = false, bool TCOND = false, bool LEAD = false>
__global__ __launch_bounds__(BOX_LANES) void k_box_prob(int M, const double *__restrict__ L, const double *__restrict__ lo,
                                                        const double *__restrict__ hi, const double *__restrict__ shift, int B, int b0,
                                                        const uint64_t *__restrict__ seeds, int r0, const uint32_t *__restrict__ streams,
                                                        const uint64_t *__restrict__ table, int table_rows, int64_t first, int64_t n,
                                                        int64_t blk0, int64_t call_blk0, int64_t call_blocks,
                                                        double *__restrict__ partials, double *__restrict__ f_out, int64_t ldf,
                                                        int64_t c_off, double *__restrict__ z_out, double *__restrict__ u_out,
                                                        const double *__restrict__ mix, const double *__restrict__ scl,
                                                        int64_t fstride) {
    extern __shared__ double ys[];                     // y[k][lane]
    const int lane = threadIdx.x;
    const int b = b0 + (int)blockIdx.y, r = r0 + (int)blockIdx.z;
    L += (int64_t)b * fstride;                         // the box's own factor (the _pf_ entries); uniform over the wave as before
    const int64_t a = blk0 + blockIdx.x;
    const int64_t j = (a << 6) | lane;
    const bool active = j >= first && j < first + n;
    const double *lo_b = lo + (int64_t)b * M, *hi_b = hi + (int64_t)b * M;
    const double *sh_b = !LEAD && shift ? shift + (int64_t)b * M : nullptr;
    const uint64_t seed = seeds[r];
    const uint64_t *tab = SOBOL ? table + (int64_t)r * table_rows * SOBOL_ROW : nullptr;
    double sc = 1.0;
    if constexpr (TCOP && !LEAD) sc = mix[((int64_t)r * gridDim.x + blockIdx.x) * BOX_LANES + lane];
    if constexpr (TCOND)
        if (scl) sc = __dmul_rn(scl[b], sc);
    double f = 1.0;
    if constexpr (LEAD) {
        const int64_t at = (((int64_t)r * B + b) * gridDim.x + blockIdx.x) * BOX_LANES + lane;
        const double vl = scl[at];
        sc = mix[at];
        if (M > 1) ys[lane] = vl / sc;
        if constexpr (DRAWS) {
            const double z = fmin(fmax(__dmul_rn(vl, L[0]), lo_b[0]), hi_b[0]);
            const int64_t to = ((int64_t)r * B + b) * M * ldf + (j - first - c_off);
            if (active && u_out) u_out[to] = z;
            if (active) z_out[to] = z;
        }
    }
    for (int i = LEAD ? 1 : 0; i < M; ++i) {
        const double *Li = L + (int64_t)i * M;
        double s = !TCOND && sh_b ? sh_b[i] : 0.0;
        for (int k = 0; k < i; ++k) s = __dadd_rn(s, __dmul_rn(Li[k], ys[k * BOX_LANES + lane]));
        double lt = lo_b[i], ht = hi_b[i];
        if constexpr (TCOND)
            if (sh_b) lt = __dsub_rn(lt, sh_b[i]), ht = __dsub_rn(ht, sh_b[i]);
        const double lii = Li[i], l = TCOP ? lt / sc : lt, h = TCOP ? ht / sc : ht;
        const double ap = (l - s) / lii, bp = (h - s) / lii;
        const bool refl = ap > 0.0;
        const double d = box_normcdf(refl ? -bp : ap), e = box_normcdf(refl ? -ap : bp);
        const double width = l < h ? e - d : 0.0;
        f *= width;
        if (DRAWS || i < M - 1) {
            double w;
            if constexpr (SOBOL) w = box_sobol_unit(tab + (int64_t)streams[i] * SOBOL_ROW, (uint64_t)a, lane);
            else w = q_uniform(seed, streams[i], (uint64_t)j);
            const double p = fmin(fmax(__dadd_rn(d, __dmul_rn(w, width)), 0x1p-1022), 1.0 - 0x1p-53);
            double y = box_normcdfinv(p);
            y = refl ? -y : y;
            if (i < M - 1) ys[i * BOX_LANES + lane] = y;
            if constexpr (DRAWS) {
                // an empty component (l >= h) gives h: max(., l) >= l >= h
                double z = fmin(fmax(__dadd_rn(s, __dmul_rn(lii, y)), l), h);
                const int64_t at = (((int64_t)r * B + b) * M + i) * ldf + (j - first - c_off);
                if constexpr (TCOP) {
                    z = __dmul_rn(z, sc);
                    if constexpr (TCOND)
                        if (sh_b) z = __dadd_rn(sh_b[i], z);
                    z = fmin(fmax(z, lo_b[i]), hi_b[i]);
                    if (active && u_out) u_out[at] = z;
                }
                if (active) z_out[at] = z;
                if (!TCOP && u_out) {
                    const double u = fmin(fmax(box_normcdf(z), 0x1p-53), 1.0 - 0x1p-53);
                    if (active) u_out[at] = u;
                }
            }
        }
    }
    if constexpr (LEAD) f = __dmul_rn(shift[b], f);
    if (active && f_out) f_out[((int64_t)r * B + b) * ldf + (j - first - c_off)] = f;
    double v = active ? f : 0.0;
#pragma unroll
    for (int o = BOX_LANES / 2; o; o >>= 1) v += __shfl_xor(v, o);
    // M = 1 uses no point: every lane holds e - d, and k_box_mean hands it on as it is
    // (under TCOP the one width depends on the point's mixing scale: the tree as for every other M; under LEAD it is W0 again)
    if (lane == 0) partials[((int64_t)r * B + b) * call_blocks + (a - call_blk0)] = M == 1 && (!TCOP || LEAD) ? f : v;
}

__global__ __launch_bounds__(BOX_MEAN_THREADS) void k_box_mean(const double *__restrict__ partials, int64_t call_blocks, int64_t n,
                                                               int single, double *__restrict__ mean) {
    __shared__ double sh[BOX_MEAN_THREADS];
    const int t = threadIdx.x;
    const double *p = partials + (int64_t)blockIdx.x * call_blocks;
    double acc = 0.0;
    for (int64_t k = t; k < call_blocks; k += BOX_MEAN_THREADS) acc += p[k];
    sh[t] = acc;
    __syncthreads();
    for (int s = BOX_MEAN_THREADS / 2; s; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    if (t == 0) mean[blockIdx.x] = single ? p[0] : sh[0] / (double)n;
}

static int box_prob(const char *fn, int32_t M, const double *L, int32_t B, const double *lo, const double *hi, const double *shift, int32_t R,
                    const uint64_t *seeds, const uint32_t *streams, int64_t first, int64_t n, int32_t flags, double *mean, double *f_out,
                    int mem_kind, bool draws = false, double *z_out = nullptr, double *u_out = nullptr, const double *dof = nullptr,
                    uint32_t mix_stream = 0, double *s_out = nullptr, const double *dof_mix = nullptr, const double *scale = nullptr,
                    bool lead = false, double *lead_out = nullptr, int64_t factor_stride = 0) {
    const std::string e(fn);
    const bool tcop = dof != nullptr;                  // the t entries: *dof degrees of freedom, the mixing stream, s_out [R][n] or NULL
    // the tc entries: a conditional law, *dof_mix degrees of freedom of the mixing variable, shift [B][M] or NULL, scale [B] or NULL
    const bool tcond = tcop && dof_mix != nullptr;
    // the tl entries (lead, with tcop and without tcond): component 0 is drawn inside its limits, the mixing variable has *dof + 1
    // degrees of freedom given it; s_out and lead_out are [R][B][n]
    if (!rt().ready) return fail("mlmc_init has not been called (no HIP device bound)");
    if (tcop && tcop_check_dof(fn, *dof)) return 1;
    if (tcond && tcop_check_dof(fn, *dof_mix, TCOP_MAX_DOF_MIX, "dof_mix")) return 1;
    if (M < 1) return fail(e + ": M < 1");
    if (M > MLMC_BOX_PROB_MAX_M) return fail(e + ": M = " + std::to_string(M) + " is above the cap " + std::to_string(MLMC_BOX_PROB_MAX_M));
    if (B < 1) return fail(e + ": B < 1");
    if (R < 1) return fail(e + ": R < 1");
    if (!L || !lo || !hi || !seeds || !mean || (draws && (!f_out || !z_out))) return fail(e + ": null argument");
    if (mem_kind != MLMC_HOST && mem_kind != MLMC_DEVICE) return fail(e + ": bad mem_kind");
    if (flags & ~(MLMC_SAMPLE_ANTITHETIC | MLMC_SAMPLE_SOBOL)) return fail(e + ": unknown bits in flags");
    if (flags & MLMC_SAMPLE_ANTITHETIC) return fail(e + ": MLMC_SAMPLE_ANTITHETIC does not apply to this entry");
    const bool sobol = flags & MLMC_SAMPLE_SOBOL;
    if (n < 1) return fail(e + ": n < 1");
    if (first < 0) return fail(e + ": first < 0");
    if (first > SOBOL_MAX_INDEX - n) return fail(e + ": first + n is beyond 2^52");
    // the _pf_ entries: box b reads the factor L + b * factor_stride (0: all boxes share one); every factor is checked
    if (factor_stride != 0 && factor_stride < (int64_t)M * M)
        return fail(e + ": factor_stride = " + std::to_string(factor_stride) + " must be 0 (one shared factor) or at least M * M = " +
                    std::to_string((int64_t)M * M));
    const int nf = factor_stride ? B : 1;
    for (int g = 0; g < nf; ++g) {
        const double *Lg = L + (size_t)g * (size_t)factor_stride;
        const std::string at = factor_stride ? ": box " + std::to_string(g) + ", factor row " : ": factor row ";
        for (int i = 0; i < M; ++i) {
            const double dg = Lg[(size_t)i * M + i];
            if (!std::isfinite(dg) || !(dg > 0.0))
                return fail(e + at + std::to_string(i) + ": the diagonal entry must be finite and positive");
            for (int k = 0; k < i; ++k)
                if (!std::isfinite(Lg[(size_t)i * M + k]))
                    return fail(e + at + std::to_string(i) + ": entry " + std::to_string(k) + " is not finite");
        }
    }
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < M; ++i) {
            const size_t at = (size_t)b * M + i;
            if (std::isnan(lo[at]) || std::isnan(hi[at]))
                return fail(e + ": box " + std::to_string(b) + ", component " + std::to_string(i) + ": a limit is NaN");
            if (shift && !std::isfinite(shift[at]))
                return fail(e + ": box " + std::to_string(b) + ", component " + std::to_string(i) + ": the shift is not finite");
        }
    if (tcond && scale)
        for (int b = 0; b < B; ++b)
            if (!std::isfinite(scale[b]) || !(scale[b] > 0.0))
                return fail(e + ": box " + std::to_string(b) + ": the scale must be finite and positive");
    // the coordinates: streams (Philox), or the rows of the call's distinct dimensions, one table per seed (MLMC_SAMPLE_SOBOL)
    // the draws take one more coordinate for the last component; the lead of the tl entries has coordinate 0 even where M = 1
    const int nc = draws ? M : lead ? std::max(M - 1, 1) : M - 1;
    // the t entries: the mixing variable is one more coordinate, behind the chain's, in the same table
    const int nd = nc + (tcop ? 1 : 0);
    std::vector<uint32_t> dims;
    if (tcop) {
        for (int i = 0; i < nc; ++i) {
            dims.push_back(streams ? streams[i] : (uint32_t)i);
            if (dims[i] == mix_stream) return fail(e + ": mix_stream equals the stream of coordinate " + std::to_string(i));
        }
        if (sobol && mix_stream >= 1024) return fail(e + ": mix_stream " + std::to_string(mix_stream) + " is not a Sobol' dimension below 1024");
        dims.push_back(mix_stream);
        streams = dims.data();
    }
    std::vector<uint32_t> coord((size_t)nd);
    std::vector<uint64_t> tables;
    int table_rows = 0;
    if (sobol && nd > 0) {
        std::vector<uint64_t> tab;
        std::vector<uint32_t> slot;
        for (int r = 0; r < R; ++r) {
            if (sobol_call_table(fn, "coordinate", seeds[r], streams, nd, tab, slot)) return 1;
            tables.insert(tables.end(), tab.begin(), tab.end());
        }
        table_rows = (int)(tab.size() / SOBOL_ROW);
        coord = slot;
    } else
        for (int i = 0; i < nd; ++i) coord[i] = streams ? streams[i] : (uint32_t)i;

    const int64_t call_blk0 = first >> 6, call_blocks = ((first + n - 1) >> 6) - call_blk0 + 1;
    const size_t pairs = (size_t)R * (size_t)B;
    if ((double)pairs * (double)call_blocks * sizeof(double) > (double)BOX_PARTIAL_BYTES)
        return fail(e + ": R * B * n / 64 partial sums exceed 1 GiB: split the boxes or the seeds across calls (no value depends on it)");
    // blocks of a launch: all of them, or what keeps the staged integrand within BOX_F_BYTES (MLMC_BOX_PROB_BLOCK_POINTS in the
    // environment, read per call, sets the points of a launch, rounded up to whole blocks: a test aid, no value depends on it)
    const bool stage = f_out && mem_kind == MLMC_HOST;
    // staged rows of a pair: the integrand, and with draws the M rows of z and of u
    const size_t zrows = draws ? pairs * (size_t)M : 0, urows = u_out ? zrows : 0, rows = pairs + zrows + urows;
    int64_t lb = std::min<int64_t>(call_blocks, 0x7fffffff);
    // the t entries keep the mixing scales of a launch, one row per seed, within the same bytes; the tl entries also the lead score
    // and the conditioned scale, one row per pair each
    if (stage || tcop) {
        lb = std::min<int64_t>(lb, (int64_t)(BOX_F_BYTES / (sizeof(double) * BOX_LANES *
                                                            ((stage ? rows : 0) + (tcop ? (size_t)R : 0) + (lead ? 2 * pairs : 0)))));
        if (lb < 1 && !stage && lead)
            return fail(e + ": the lead scores of one block of 64 points of R * B pairs exceed 192 MiB: split the boxes or the seeds across calls");
        if (lb < 1 && !stage) return fail(e + ": the mixing scales of one block of 64 points of R seeds exceed 192 MiB: split the seeds across calls");
        if (lb < 1)
            return fail(e + (draws ? ": the draws" : ": the integrand") +
                        " of one block of 64 points of R * B pairs exceed" + (draws ? "" : "s") +
                        " 192 MiB: split the boxes or the seeds across calls");
    }
    if (const char *env = std::getenv("MLMC_BOX_PROB_BLOCK_POINTS")) {
        const long long v = std::atoll(env);
        if (v > 0) lb = std::min<int64_t>(lb, (v + BOX_LANES - 1) / BOX_LANES);
    }
    const int64_t ldf = stage ? lb * BOX_LANES : n;

    // what goes up: L | lo | hi | shift | scale | seeds | tables | coordinates (uint32)
    // (the factors go up packed: M * M doubles apart on the device whatever the caller's stride)
    const size_t nL = (size_t)nf * M * M, nbx = (size_t)B * M, nsh = shift ? nbx : 0, ntab = tables.size(), nco = ((size_t)nd + 1) / 2;
    const size_t nsc = tcond && scale ? (size_t)B : 0;
    const size_t n_in = nL + 2 * nbx + nsh + nsc + (size_t)R + ntab + nco;
    std::vector<double> packed(n_in);
    double *q = packed.data();
    for (int g = 0; g < nf; ++g) std::memcpy(q, L + (size_t)g * (size_t)factor_stride, sizeof(double) * (size_t)M * M), q += (size_t)M * M;
    std::memcpy(q, lo, sizeof(double) * nbx), q += nbx;
    std::memcpy(q, hi, sizeof(double) * nbx), q += nbx;
    if (nsh) std::memcpy(q, shift, sizeof(double) * nsh), q += nsh;
    if (nsc) std::memcpy(q, scale, sizeof(double) * nsc), q += nsc;
    std::memcpy(q, seeds, sizeof(uint64_t) * (size_t)R), q += R;
    if (ntab) std::memcpy(q, tables.data(), sizeof(uint64_t) * ntab), q += ntab;
    if (nd) std::memcpy(q, coord.data(), sizeof(uint32_t) * (size_t)nd);

    const size_t b_in = mm_align(sizeof(double) * n_in), b_part = mm_align(sizeof(double) * pairs * (size_t)call_blocks);
    const size_t b_mean = mm_align(sizeof(double) * pairs), b_f = stage ? mm_align(sizeof(double) * pairs * (size_t)ldf) : 0;
    const size_t b_z = stage ? mm_align(sizeof(double) * zrows * (size_t)ldf) : 0, b_u = stage ? mm_align(sizeof(double) * urows * (size_t)ldf) : 0;
    const size_t b_s = tcop ? mm_align(sizeof(double) * (size_t)R * (size_t)lb * BOX_LANES) : 0;
    // the tl entries: W0 | d [B], then v and sc [R * B][64 lb]
    const size_t b_w = lead ? mm_align(sizeof(double) * 2 * (size_t)B) : 0;
    const size_t b_v = lead ? mm_align(sizeof(double) * pairs * (size_t)lb * BOX_LANES) : 0;
    static MultiWorkspace ws;
    if (ws.reserve(b_in + b_part + b_mean + b_f + b_z + b_u + b_s + b_w + 2 * b_v)) return 1;
    double *d_s = tcop ? (double *)(ws.dev + b_in + b_part + b_mean + b_f + b_z + b_u) : nullptr;
    double *d_w = lead ? (double *)(ws.dev + b_in + b_part + b_mean + b_f + b_z + b_u + b_s) : nullptr;
    double *d_v = lead ? (double *)(ws.dev + b_in + b_part + b_mean + b_f + b_z + b_u + b_s + b_w) : nullptr;
    double *d_sc = lead ? (double *)(ws.dev + b_in + b_part + b_mean + b_f + b_z + b_u + b_s + b_w + b_v) : nullptr;
    double *d_in = (double *)ws.dev, *d_part = (double *)(ws.dev + b_in), *d_mean = (double *)(ws.dev + b_in + b_part);
    double *d_f = stage ? (double *)(ws.dev + b_in + b_part + b_mean) : f_out;
    double *d_z = stage && draws ? (double *)(ws.dev + b_in + b_part + b_mean + b_f) : z_out;
    double *d_u = stage && u_out ? (double *)(ws.dev + b_in + b_part + b_mean + b_f + b_z) : u_out;
    hipStream_t st = rt().stream;
    MLMC_HIP_CHECK(hipMemcpyAsync(d_in, packed.data(), sizeof(double) * n_in, hipMemcpyHostToDevice, st));
    const double *d_L = d_in, *d_lo = d_L + nL, *d_hi = d_lo + nbx, *d_shift = nsh ? d_hi + nbx : nullptr;
    const double *d_scale = nsc ? d_hi + nbx + nsh : nullptr;
    const uint64_t *d_seeds = (const uint64_t *)(d_hi + nbx + nsh + nsc), *d_tab = d_seeds + R;
    const uint32_t *d_coord = (const uint32_t *)(d_tab + ntab);

    const int64_t d_fstride = factor_stride ? (int64_t)M * M : 0;
    const size_t lds = sizeof(double) * BOX_LANES * (size_t)(M - 1);
    const auto kernel = lead  ? (draws ? (sobol ? k_box_prob<true, true, true, false, true> : k_box_prob<false, true, true, false, true>)
                                       : (sobol ? k_box_prob<true, false, true, false, true> : k_box_prob<false, false, true, false, true>))
                      : tcond ? (draws ? (sobol ? k_box_prob<true, true, true, true> : k_box_prob<false, true, true, true>)
                                       : (sobol ? k_box_prob<true, false, true, true> : k_box_prob<false, false, true, true>))
                      : tcop ? (draws ? (sobol ? k_box_prob<true, true, true> : k_box_prob<false, true, true>)
                                      : (sobol ? k_box_prob<true, false, true> : k_box_prob<false, false, true>))
                             : (draws ? (sobol ? k_box_prob<true, true> : k_box_prob<false, true>)
                                      : (sobol ? k_box_prob<true, false> : k_box_prob<false, false>));
    // the CDF pass maps with the constants of dof (the marginal law of a component), the mixing kernel takes those of dof_mix
    const TCopConst tconst = tcop ? tcop_constants(*dof) : TCopConst{};
    const TCopConst tmix = tcond ? tcop_constants(*dof_mix) : lead ? tcop_constants(*dof + 1.0) : tconst;
    // the lead's weight of every box, once per call
    if (lead) cop_launch_box_lead_weights(st, tconst, (int)M, d_L, d_fstride, d_lo, d_hi, (int)B, d_w);
    for (int64_t k0 = 0; k0 < call_blocks; k0 += lb) {
        const int64_t kb = std::min(lb, call_blocks - k0);
        // the first point of the launch within the call: column 0 of the staged integrand
        const int64_t c_lo = std::max<int64_t>(((call_blk0 + k0) << 6) - first, 0);
        const int64_t c_hi = std::min<int64_t>(((call_blk0 + k0 + kb) << 6) - first, n);
        if (tcop) {
            // the mixing scales of the launch's blocks, once per (seed, point): d_s [R][64 kb]
            const int64_t j0 = (call_blk0 + k0) << 6;
            cop_launch_box_mixing(st, tmix, R, d_seeds, coord[nc], sobol ? d_tab : nullptr, table_rows, j0, kb * BOX_LANES, first, n, d_s);
            if (lead) {
                // v and sc of the launch's blocks for every pair: [R * B][64 kb], from the scales g0 [R][64 kb] just made
                cop_launch_box_lead(st, tconst, (int)M, d_L, d_fstride, d_lo, d_hi, (int)B, R, d_seeds, coord[0], sobol ? d_tab : nullptr, table_rows, j0,
                                    kb * BOX_LANES, first, n, d_s, d_w, d_v, d_sc);
                const hipMemcpyKind kind = mem_kind == MLMC_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
                if (s_out)
                    MLMC_HIP_CHECK(hipMemcpy2DAsync(s_out + c_lo, sizeof(double) * (size_t)n, d_sc + (first + c_lo - j0),
                                                    sizeof(double) * (size_t)(kb * BOX_LANES), sizeof(double) * (size_t)(c_hi - c_lo), pairs,
                                                    kind, st));
                if (lead_out)
                    MLMC_HIP_CHECK(hipMemcpy2DAsync(lead_out + c_lo, sizeof(double) * (size_t)n, d_v + (first + c_lo - j0),
                                                    sizeof(double) * (size_t)(kb * BOX_LANES), sizeof(double) * (size_t)(c_hi - c_lo), pairs,
                                                    kind, st));
            } else if (s_out)
                MLMC_HIP_CHECK(hipMemcpy2DAsync(s_out + c_lo, sizeof(double) * (size_t)n, d_s + (first + c_lo - j0),
                                                sizeof(double) * (size_t)(kb * BOX_LANES), sizeof(double) * (size_t)(c_hi - c_lo), (size_t)R,
                                                mem_kind == MLMC_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
        }
        for (int r0 = 0; r0 < R; r0 += 65535)
            for (int b0 = 0; b0 < B; b0 += 65535) {
                const dim3 grid((unsigned)kb, (unsigned)std::min(B - b0, 65535), (unsigned)std::min(R - r0, 65535));
                hipLaunchKernelGGL(kernel, grid, dim3(BOX_LANES), lds, st, (int)M, d_L, d_lo, d_hi, lead ? (const double *)d_w : d_shift, (int)B,
                                   b0, d_seeds, r0, d_coord, d_tab, table_rows, first, n, call_blk0 + k0, call_blk0, call_blocks, d_part,
                                   d_f, ldf, stage ? c_lo : (int64_t)0, d_z, d_u, (const double *)(lead ? d_sc : d_s),
                                   lead ? (const double *)d_v : d_scale, d_fstride);
            }
        // the CDF pass of the t draws: the rows of u hold the t scores of the launch's columns and are mapped in place
        if (tcop && u_out) cop_launch_t_map(st, tconst, (int)urows, c_hi - c_lo, d_u + (stage ? 0 : c_lo), ldf);
        MLMC_HIP_CHECK(hipGetLastError());
        if (stage) {
            MLMC_HIP_CHECK(hipMemcpy2DAsync(f_out + c_lo, sizeof(double) * (size_t)n, d_f, sizeof(double) * (size_t)ldf,
                                            sizeof(double) * (size_t)(c_hi - c_lo), pairs, hipMemcpyDeviceToHost, st));
            if (draws)
                MLMC_HIP_CHECK(hipMemcpy2DAsync(z_out + c_lo, sizeof(double) * (size_t)n, d_z, sizeof(double) * (size_t)ldf,
                                                sizeof(double) * (size_t)(c_hi - c_lo), zrows, hipMemcpyDeviceToHost, st));
            if (u_out)
                MLMC_HIP_CHECK(hipMemcpy2DAsync(u_out + c_lo, sizeof(double) * (size_t)n, d_u, sizeof(double) * (size_t)ldf,
                                                sizeof(double) * (size_t)(c_hi - c_lo), urows, hipMemcpyDeviceToHost, st));
        }
    }
    hipLaunchKernelGGL(k_box_mean, dim3((unsigned)pairs), dim3(BOX_MEAN_THREADS), 0, st, (const double *)d_part, call_blocks, n,
                       (int)(M == 1 && (!tcop || lead)), d_mean);
    MLMC_HIP_CHECK(hipGetLastError());
    MLMC_HIP_CHECK(hipMemcpyAsync(mean, d_mean, sizeof(double) * pairs, hipMemcpyDeviceToHost, st));
    MLMC_HIP_CHECK(wait_stream(st));
    return 0;
}

}  // namespace mlmc

using namespace mlmc;

extern "C" {

int mlmc_copula_box_prob_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, const double *shift, int32_t R,
                               const uint64_t *seeds, const uint32_t *streams, int64_t first, int64_t n, int32_t flags, double *mean,
                               double *f_out, int mem_kind) {
    MLMC_API_GUARD;
    return box_prob("mlmc_copula_box_prob_batch", M, L, B, lo, hi, shift, R, seeds, streams, first, n, flags, mean, f_out, mem_kind);
}

int mlmc_copula_box_prob_pf_batch(int32_t M, const double *L, int64_t factor_stride, int32_t B, const double *lo, const double *hi,
                                  const double *shift, int32_t R, const uint64_t *seeds, const uint32_t *streams, int64_t first, int64_t n,
                                  int32_t flags, double *mean, double *f_out, int mem_kind) {
    MLMC_API_GUARD;
    return box_prob("mlmc_copula_box_prob_pf_batch", M, L, B, lo, hi, shift, R, seeds, streams, first, n, flags, mean, f_out, mem_kind, false,
                    nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, false, nullptr, factor_stride);
}

int mlmc_copula_box_draws_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, const double *shift, int32_t R,
                                const uint64_t *seeds, const uint32_t *streams, int64_t first, int64_t n, int32_t flags, double *mean,
                                double *f_out, double *z_out, double *u_out, int mem_kind) {
    MLMC_API_GUARD;
    return box_prob("mlmc_copula_box_draws_batch", M, L, B, lo, hi, shift, R, seeds, streams, first, n, flags, mean, f_out, mem_kind, true,
                    z_out, u_out);
}

int mlmc_copula_box_prob_t_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, int32_t R,
                                 const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream, int64_t first, int64_t n,
                                 int32_t flags, double *mean, double *f_out, double *s_out, int mem_kind) {
    MLMC_API_GUARD;
    return box_prob("mlmc_copula_box_prob_t_batch", M, L, B, lo, hi, nullptr, R, seeds, streams, first, n, flags, mean, f_out, mem_kind, false,
                    nullptr, nullptr, &dof, mix_stream, s_out);
}

int mlmc_copula_box_prob_t_pf_batch(int32_t M, const double *L, int64_t factor_stride, int32_t B, const double *lo, const double *hi,
                                    double dof, int32_t R, const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream, int64_t first,
                                    int64_t n, int32_t flags, double *mean, double *f_out, double *s_out, int mem_kind) {
    MLMC_API_GUARD;
    return box_prob("mlmc_copula_box_prob_t_pf_batch", M, L, B, lo, hi, nullptr, R, seeds, streams, first, n, flags, mean, f_out, mem_kind,
                    false, nullptr, nullptr, &dof, mix_stream, s_out, nullptr, nullptr, false, nullptr, factor_stride);
}

int mlmc_copula_box_draws_t_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, int32_t R,
                                  const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream, int64_t first, int64_t n,
                                  int32_t flags, double *mean, double *f_out, double *z_out, double *u_out, double *s_out, int mem_kind) {
    MLMC_API_GUARD;
    return box_prob("mlmc_copula_box_draws_t_batch", M, L, B, lo, hi, nullptr, R, seeds, streams, first, n, flags, mean, f_out, mem_kind, true,
                    z_out, u_out, &dof, mix_stream, s_out);
}

int mlmc_copula_box_prob_tl_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, int32_t R,
                                  const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream, int64_t first, int64_t n,
                                  int32_t flags, double *mean, double *f_out, double *s_out, double *lead_out, int mem_kind) {
    MLMC_API_GUARD;
    return box_prob("mlmc_copula_box_prob_tl_batch", M, L, B, lo, hi, nullptr, R, seeds, streams, first, n, flags, mean, f_out, mem_kind, false,
                    nullptr, nullptr, &dof, mix_stream, s_out, nullptr, nullptr, true, lead_out);
}

int mlmc_copula_box_prob_tl_pf_batch(int32_t M, const double *L, int64_t factor_stride, int32_t B, const double *lo, const double *hi,
                                     double dof, int32_t R, const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream,
                                     int64_t first, int64_t n, int32_t flags, double *mean, double *f_out, double *s_out, double *lead_out,
                                     int mem_kind) {
    MLMC_API_GUARD;
    return box_prob("mlmc_copula_box_prob_tl_pf_batch", M, L, B, lo, hi, nullptr, R, seeds, streams, first, n, flags, mean, f_out, mem_kind,
                    false, nullptr, nullptr, &dof, mix_stream, s_out, nullptr, nullptr, true, lead_out, factor_stride);
}

int mlmc_copula_box_draws_tl_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, int32_t R,
                                   const uint64_t *seeds, const uint32_t *streams, uint32_t mix_stream, int64_t first, int64_t n,
                                   int32_t flags, double *mean, double *f_out, double *z_out, double *u_out, double *s_out,
                                   double *lead_out, int mem_kind) {
    MLMC_API_GUARD;
    return box_prob("mlmc_copula_box_draws_tl_batch", M, L, B, lo, hi, nullptr, R, seeds, streams, first, n, flags, mean, f_out, mem_kind, true,
                    z_out, u_out, &dof, mix_stream, s_out, nullptr, nullptr, true, lead_out);
}

int mlmc_copula_box_prob_tc_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, double dof_mix,
                                  const double *shift, const double *scale, int32_t R, const uint64_t *seeds, const uint32_t *streams,
                                  uint32_t mix_stream, int64_t first, int64_t n, int32_t flags, double *mean, double *f_out,
                                  double *s_out, int mem_kind) {
    MLMC_API_GUARD;
    return box_prob("mlmc_copula_box_prob_tc_batch", M, L, B, lo, hi, shift, R, seeds, streams, first, n, flags, mean, f_out, mem_kind, false,
                    nullptr, nullptr, &dof, mix_stream, s_out, &dof_mix, scale);
}

int mlmc_copula_box_draws_tc_batch(int32_t M, const double *L, int32_t B, const double *lo, const double *hi, double dof, double dof_mix,
                                   const double *shift, const double *scale, int32_t R, const uint64_t *seeds, const uint32_t *streams,
                                   uint32_t mix_stream, int64_t first, int64_t n, int32_t flags, double *mean, double *f_out,
                                   double *z_out, double *u_out, double *s_out, int mem_kind) {
    MLMC_API_GUARD;
    return box_prob("mlmc_copula_box_draws_tc_batch", M, L, B, lo, hi, shift, R, seeds, streams, first, n, flags, mean, f_out, mem_kind, true,
                    z_out, u_out, &dof, mix_stream, s_out, &dof_mix, scale);
}

}  // extern "C"
