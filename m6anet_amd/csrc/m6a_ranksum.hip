// m6a_ranksum.hip -- m6a_site_ranksum (include/m6a.h): the two-sided Mann-Whitney U test of pairs of sites, one site from each of two
// sets of read probabilities.  The counting is all-pairs and exact in integers; z comes from m6a_ranksum.h, which the host compiles too.
// The scheme -- the pair header, the tile fills, the walk and the launch, the entry point -- is m6a_pairs.h's, shared with m6a_ks.hip.
//   site_ranksum_kernel  a wavefront per pair.  The pooled sample a ++ b (N = n + m reads) is walked in chunks of 64: lane l owns
//                        pooled element c0 + l.  For every chunk both bags stream through the wavefront's LDS tile
//                        (M6A_PAIR_TILE floats, padded to whole float4s with NaN, which compares false), read back as float4
//                        broadcasts: every lane compares its element with the same four values, two VALU operations per compare.
//                        A lane counts c = the pooled elements equal to its own (tie = sum of c^2 - 1) and, where its element is
//                        of a, the b below it and equal to it.  The per-chunk counts are 32-bit (at most 2^20 each); they are
//                        folded into 64-bit sums per chunk, so nothing can overflow; three integer butterflies close the pair.
//                        No float is added anywhere.  A pair of 20 + 20 reads is one chunk and two tiles of five float4s.
// The cost is N^2 compares on one wavefront: bags of tens to a few thousand reads are what it is for.  The largest defined pair
// (N = 2^20) is computed, but takes that wavefront about a minute.
// m6a_site_signal_ranksum, behind it in this file: the same test on each of the nine columns of two sets' X [R][9].
//   site_signal_ranksum_kernel  a wavefront per pair again, lane l owning pooled ROW c0 + l with its nine values in registers.  A tile
//                        of M6A_PAIR_TILE rows of a bag is loaded once per (chunk, tile) as one contiguous run of dwords and written
//                        to LDS column-major (pair_fill_rows); the inner loop is the one above per column.  27 32-bit counters per
//                        chunk, folded into 27 64-bit sums per chunk, integer butterflies, and lanes 0..8 finish and write one
//                        column each.  DESIGN.md 7.5 has the LDS layout.
#pragma clang fp contract(off)
#include "m6a_pairs.h"

using namespace m6a_detail;

namespace {

struct RanksumArgs : PairsIn {
    int64_t *gt, *eq, *tie;           // [n_pairs] or [n_pairs][9], each may be null
    double *z;                        // the same shape
    int *err;
};

__device__ __forceinline__ unsigned long long ranksum_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v += __shfl_xor(v, h, 64);
    return v;
}

// one bag through the tile against every lane's x: eq += #{s == x}; GT: gt += #{s < x}
template <bool GT>
__device__ __forceinline__ void ranksum_stream(float *tile, const float *p, int64_t len, int lane, float x, unsigned &eq, unsigned &gt)
{
    for (int64_t t0 = 0; t0 < len; t0 += M6A_PAIR_TILE) {
        const int cnt = (int)(len - t0 < M6A_PAIR_TILE ? len - t0 : M6A_PAIR_TILE);
        pair_fill(tile, p + t0, cnt, lane);
        for (int q = 0; q < (cnt + 3) / 4; q++) {
            const float4 s = make_float4(tile[4 * q], tile[4 * q + 1], tile[4 * q + 2], tile[4 * q + 3]);   // one 16-byte broadcast
            eq += pair_one(x == s.x) + pair_one(x == s.y) + pair_one(x == s.z) + pair_one(x == s.w);
            if (GT) gt += pair_one(x > s.x) + pair_one(x > s.y) + pair_one(x > s.z) + pair_one(x > s.w);
        }
    }
}

__global__ __launch_bounds__(256) void site_ranksum_kernel(RanksumArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[M6A_PAIR_WAVES][M6A_PAIR_TILE];
    const int lane = threadIdx.x & 63, w = pair_wave();
    float *tile = lds[w];
    const int64_t step = pair_step();
    for (int64_t k = pair_first(w); k < a.n_pairs; k += step) {
        int64_t a0, a1, b0, b1;
        const bool bad = !pair_bags(a, k, a0, a1, b0, b1);
        const int64_t n = a1 - a0, m = b1 - b0, N = n + m;
        m6a_ranksum::Result r = m6a_ranksum::undefined();
        if (bad) {
            if (lane == 0) atomicExch(a.err, 5);
        } else if (!m6a_ranksum::undefined_sizes(n, m)) {
            const float *pa = a.v_a + a0, *pb = a.v_b + b0;
            unsigned long long gt = 0, eq = 0, tie = 0;
            bool nan = false;
            for (int64_t c0 = 0; c0 < N; c0 += 64) {
                const int64_t i = c0 + lane;
                const bool own = i < N, of_a = i < n;
                const float x = own ? (of_a ? pa[i] : pb[i - n]) : __builtin_nanf("");
                nan = nan || (own && x != x);
                unsigned ceq = 0, cgt = 0, ceb = 0;
                ranksum_stream<false>(tile, pa, n, lane, x, ceq, cgt);
                if (c0 < n) ranksum_stream<true>(tile, pb, m, lane, x, ceb, cgt);   // uniform: only a chunk that holds elements of a counts the b below them
                else ranksum_stream<false>(tile, pb, m, lane, x, ceb, cgt);
                const unsigned long long c = (unsigned long long)ceq + ceb;
                if (own) tie += c * c - 1ull;                   // (a NaN element has c = 0; the pair is undefined then)
                if (of_a) { gt += cgt; eq += ceb; }
            }
            gt = ranksum_wave_sum(gt);
            eq = ranksum_wave_sum(eq);
            tie = ranksum_wave_sum(tie);
            if (__ballot(nan) == 0ull)
                r = {(int64_t)gt, (int64_t)eq, (int64_t)tie, m6a_ranksum::finish(n, m, (int64_t)gt, (int64_t)eq, (int64_t)tie)};
        }
        if (lane == 0) {
            if (a.gt) a.gt[k] = r.gt;
            if (a.eq) a.eq[k] = r.eq;
            if (a.tie) a.tie[k] = r.tie;
            a.z[k] = r.z;
        }
    }
}

// ---- m6a_site_signal_ranksum: the test above on each of the nine columns of X [R][9] ------------------------------------------------

// This kernel keeps its three compare loops written out.  As one ranksum_stream<GT> on rows its build takes 192 VGPRs and spills 89
// SGPRs where these loops take 191 and 38; with only the q loop as a template it keeps 191 VGPRs and was measured 4 % and 14 % slower
// 
__global__ __launch_bounds__(256) void site_signal_ranksum_kernel(RanksumArgs a)
{
    constexpr int C = M6A_PAIR_COLS;
    __shared__ __attribute__((aligned(16))) float lds[M6A_PAIR_WAVES][C * M6A_PAIR_STRIDE];
    const int lane = threadIdx.x & 63, w = pair_wave();
    float *tile = lds[w];
    const int64_t step = pair_step();
    for (int64_t k = pair_first(w); k < a.n_pairs; k += step) {
        int64_t a0, a1, b0, b1;
        const bool bad = !pair_bags(a, k, a0, a1, b0, b1);
        const int64_t n = a1 - a0, m = b1 - b0, N = n + m;
        m6a_ranksum::Result r = m6a_ranksum::undefined();      // lane c < 9: column c of the pair
        if (bad) {
            if (lane == 0) atomicExch(a.err, 6);
        } else if (!m6a_ranksum::undefined_sizes(n, m)) {
            const float *pa = a.v_a + a0 * C, *pb = a.v_b + b0 * C;
            unsigned long long gt[C], eq[C], tie[C];
#pragma unroll
            for (int c = 0; c < C; c++) gt[c] = eq[c] = tie[c] = 0;
            unsigned nan = 0;                                   // bit c: a NaN in column c of a row this lane owned
            for (int64_t c0 = 0; c0 < N; c0 += 64) {
                const int64_t i = c0 + lane;
                const bool own = i < N, of_a = i < n;
                const float *row = !own ? pa : of_a ? pa + i * C : pb + (i - n) * C;   // (pa: a row that exists, read by no one)
                float x[C];
                unsigned ceq[C], cgt[C], ceb[C];
#pragma unroll
                for (int c = 0; c < C; c++) {
                    x[c] = own ? row[c] : __builtin_nanf("");
                    if (own && x[c] != x[c]) nan |= 1u << c;
                    ceq[c] = cgt[c] = ceb[c] = 0;
                }
                const bool chunk_has_a = c0 < n;                // uniform: only such a chunk counts the b below its rows
                for (int64_t t0 = 0; t0 < n; t0 += M6A_PAIR_TILE) {
                    const int cnt = (int)(n - t0 < M6A_PAIR_TILE ? n - t0 : M6A_PAIR_TILE);
                    pair_fill_rows(tile, pa + t0 * C, cnt, lane);
                    for (int q = 0; q < (cnt + 3) / 4; q++) {
#pragma unroll
                        for (int c = 0; c < C; c++) {
                            const float4 s = *reinterpret_cast<const float4 *>(tile + c * M6A_PAIR_STRIDE + 4 * q);   // one 16-byte broadcast
                            ceq[c] += pair_one(x[c] == s.x) + pair_one(x[c] == s.y) + pair_one(x[c] == s.z) + pair_one(x[c] == s.w);
                        }
                    }
                }
                for (int64_t t0 = 0; t0 < m; t0 += M6A_PAIR_TILE) {
                    const int cnt = (int)(m - t0 < M6A_PAIR_TILE ? m - t0 : M6A_PAIR_TILE);
                    pair_fill_rows(tile, pb + t0 * C, cnt, lane);
                    if (chunk_has_a) {
                        for (int q = 0; q < (cnt + 3) / 4; q++) {
#pragma unroll
                            for (int c = 0; c < C; c++) {
                                const float4 s = *reinterpret_cast<const float4 *>(tile + c * M6A_PAIR_STRIDE + 4 * q);
                                ceb[c] += pair_one(x[c] == s.x) + pair_one(x[c] == s.y) + pair_one(x[c] == s.z) + pair_one(x[c] == s.w);
                                cgt[c] += pair_one(x[c] > s.x) + pair_one(x[c] > s.y) + pair_one(x[c] > s.z) + pair_one(x[c] > s.w);
                            }
                        }
                    } else {
                        for (int q = 0; q < (cnt + 3) / 4; q++) {
#pragma unroll
                            for (int c = 0; c < C; c++) {
                                const float4 s = *reinterpret_cast<const float4 *>(tile + c * M6A_PAIR_STRIDE + 4 * q);
                                ceb[c] += pair_one(x[c] == s.x) + pair_one(x[c] == s.y) + pair_one(x[c] == s.z) + pair_one(x[c] == s.w);
                            }
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const unsigned long long t = (unsigned long long)ceq[c] + ceb[c];
                    if (own) tie[c] += t * t - 1ull;            // (a NaN value has t = 0; its column is undefined then)
                    if (of_a) { gt[c] += cgt[c]; eq[c] += ceb[c]; }
                }
            }
            unsigned long long g = 0, e = 0, t = 0;
#pragma unroll
            for (int c = 0; c < C; c++) {                       // every lane holds the pair's sums; lane c keeps column c's
                const unsigned long long sg = ranksum_wave_sum(gt[c]), se = ranksum_wave_sum(eq[c]), st = ranksum_wave_sum(tie[c]);
                if (lane == c) { g = sg; e = se; t = st; }
            }
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1) nan |= (unsigned)__shfl_xor((int)nan, h, 64);   // (as a helper in m6a_pairs.h it moves this build)
            if (lane < C && !((nan >> lane) & 1u))
                r = {(int64_t)g, (int64_t)e, (int64_t)t, m6a_ranksum::finish(n, m, (int64_t)g, (int64_t)e, (int64_t)t)};
        }
        if (lane < C) {
            const int64_t at = k * C + lane;
            if (a.gt) a.gt[at] = r.gt;
            if (a.eq) a.eq[at] = r.eq;
            if (a.tie) a.tie[at] = r.tie;
            a.z[at] = r.z;
        }
    }
}

// both entry points: z is required, the three counts are not
int site_ranksum_call(m6a_ctx *c, int cols, const float *v_a, const int64_t *off_a, int64_t n_sites_a, const float *v_b, const int64_t *off_b,
                      int64_t n_sites_b, const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs, int64_t *gt, int64_t *eq,
                      int64_t *tie, double *z, const char *sentence)
{
    return pair_call(c, cols, v_a, off_a, n_sites_a, v_b, off_b, n_sites_b, pair_a, pair_b, n_pairs, {gt, eq, tie, z}, {false, false, false, true},
                     sentence, [c, cols](const PairsIn &in, void *const *o) {
                         return pair_launch(c, cols == 1 ? site_ranksum_kernel : site_signal_ranksum_kernel,
                                            RanksumArgs{in, (int64_t *)o[0], (int64_t *)o[1], (int64_t *)o[2], (double *)o[3], c->d_err});
                     });
}

}  // namespace

extern "C" int m6a_site_ranksum(m6a_ctx *c, const float *prob_a, const int64_t *off_a, int64_t n_sites_a,
                                const float *prob_b, const int64_t *off_b, int64_t n_sites_b,
                                const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs,
                                int64_t *gt, int64_t *eq, int64_t *tie, double *z)
{
    return site_ranksum_call(c, 1, prob_a, off_a, n_sites_a, prob_b, off_b, n_sites_b, pair_a, pair_b, n_pairs, gt, eq, tie, z,
                             "prob_a, off_a, prob_b, off_b, pair_a, pair_b, gt, eq, tie, z must be all host or all device pointers");
}

extern "C" int m6a_site_signal_ranksum(m6a_ctx *c, const float *X_a, const int64_t *off_a, int64_t n_sites_a,
                                       const float *X_b, const int64_t *off_b, int64_t n_sites_b,
                                       const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs,
                                       int64_t *gt, int64_t *eq, int64_t *tie, double *z)
{
    return site_ranksum_call(c, M6A_PAIR_COLS, X_a, off_a, n_sites_a, X_b, off_b, n_sites_b, pair_a, pair_b, n_pairs, gt, eq, tie, z,
                             "X_a, off_a, X_b, off_b, pair_a, pair_b, gt, eq, tie, z must be all host or all device pointers");
}
