// m6a_ranksum.hip -- m6a_site_ranksum (include/m6a.h): the two-sided Mann-Whitney U test of pairs of sites, one site from each of two
// sets of read probabilities.  The counting is all-pairs and exact in integers; z comes from m6a_ranksum.h, which the host compiles too.
//   site_ranksum_kernel  a wavefront per pair.  The pooled sample a ++ b (N = n + m reads) is walked in chunks of 64: lane l owns
//                        pooled element c0 + l.  For every chunk both bags stream through the wavefront's LDS tile
//                        (M6A_RANKSUM_TILE floats, padded to whole float4s with NaN, which compares false), read back as float4
//                        broadcasts: every lane compares its element with the same four values, two VALU operations per compare.
//                        A lane counts c = the pooled elements equal to its own (tie = sum of c^2 - 1) and, where its element is
//                        of a, the b below it and equal to it.  The per-chunk counts are 32-bit (at most 2^20 each); they are
//                        folded into 64-bit sums per chunk, so nothing can overflow; three integer butterflies close the pair.
//                        No float is added anywhere.  A pair of 20 + 20 reads is one chunk and two tiles of five float4s.
// The cost is N^2 compares on one wavefront: bags of tens to a few thousand reads are what it is for.  The largest defined pair
// (N = 2^20) is computed, but takes that wavefront about a minute.
// m6a_site_signal_ranksum, behind it in this file: the same test on each of the nine columns of two sets' X [R][9].
//   site_signal_ranksum_kernel  a wavefront per pair again, lane l owning pooled ROW c0 + l with its nine values in registers.  A tile
//                        of M6A_SIGNAL_TILE rows of a bag is loaded once per (chunk, tile) as one contiguous run of dwords (a row is
//                        36 bytes, so no wider load has an alignment to rely on) and written to LDS column-major; the inner loop is
//                        the one above per column.  27 32-bit counters per chunk, folded into 27 64-bit sums per chunk, integer
//                        butterflies, and lanes 0..8 finish and write one column each.  DESIGN.md 7.5 has the LDS layout.
#pragma clang fp contract(off)
#include "m6a_ctx.h"
#include "m6a_ranksum.h"

using namespace m6a_detail;

#define M6A_RANKSUM_TILE 256          // floats per wavefront in LDS: 1 KB, 4 KB per block -- occupancy stays with the registers

namespace {

struct RanksumArgs {
    const float *prob_a, *prob_b;     // [off_a[n_sites_a]], [off_b[n_sites_b]]
    const int64_t *off_a, *off_b;     // [n_sites + 1]
    const int64_t *pair_a, *pair_b;   // [n_pairs] or null: the identity
    int64_t n_sites_a, n_sites_b, n_pairs;
    int64_t *gt, *eq, *tie;           // [n_pairs], each may be null
    double *z;                        // [n_pairs]
    int *err;
};

// cnt <= M6A_RANKSUM_TILE floats from p into the tile, NaN up to the next multiple of 4; ordered against the reads around it
__device__ __forceinline__ void ranksum_fill(float *tile, const float *p, int cnt, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < M6A_RANKSUM_TILE / 64; k++) {
        if (k * 64 >= cnt) break;                               // uniform
        const int j = k * 64 + lane;
        tile[j] = j < cnt ? p[j] : __builtin_nanf("");
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned long long ranksum_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v += __shfl_xor(v, h, 64);
    return v;
}

__global__ __launch_bounds__(256) void site_ranksum_kernel(RanksumArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[4][M6A_RANKSUM_TILE];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *tile = lds[w];
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t k = (int64_t)blockIdx.x * 4 + w; k < a.n_pairs; k += n_waves) {
        const int64_t ia = a.pair_a ? a.pair_a[k] : k, ib = a.pair_b ? a.pair_b[k] : k;
        bool bad = ia < 0 || ia >= a.n_sites_a || ib < 0 || ib >= a.n_sites_b;
        int64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
        if (!bad) {                                             // nothing is read through an index or an offset before it is checked
            a0 = a.off_a[ia]; a1 = a.off_a[ia + 1];
            b0 = a.off_b[ib]; b1 = a.off_b[ib + 1];
            bad = a0 < 0 || a1 < a0 || a1 > a.off_a[a.n_sites_a] || b0 < 0 || b1 < b0 || b1 > a.off_b[a.n_sites_b];
        }
        const int64_t n = a1 - a0, m = b1 - b0, N = n + m;
        m6a_ranksum::Result r = m6a_ranksum::undefined();
        if (bad) {
            if (lane == 0) atomicExch(a.err, 5);
        } else if (!m6a_ranksum::undefined_sizes(n, m)) {
            const float *pa = a.prob_a + a0, *pb = a.prob_b + b0;
            unsigned long long gt = 0, eq = 0, tie = 0;
            bool nan = false;
            for (int64_t c0 = 0; c0 < N; c0 += 64) {
                const int64_t i = c0 + lane;
                const bool own = i < N, of_a = i < n;
                const float x = own ? (of_a ? pa[i] : pb[i - n]) : __builtin_nanf("");
                nan = nan || (own && x != x);
                const bool chunk_has_a = c0 < n;                // uniform: only such a chunk counts the b below its elements
                unsigned ceq = 0, cgt = 0, ceb = 0;
                for (int64_t t0 = 0; t0 < n; t0 += M6A_RANKSUM_TILE) {
                    const int cnt = (int)(n - t0 < M6A_RANKSUM_TILE ? n - t0 : M6A_RANKSUM_TILE);
                    ranksum_fill(tile, pa + t0, cnt, lane);
                    for (int q = 0; q < (cnt + 3) / 4; q++) {
                        const float4 s = make_float4(tile[4 * q], tile[4 * q + 1], tile[4 * q + 2], tile[4 * q + 3]);   // one 16-byte broadcast
                        ceq += (x == s.x ? 1u : 0u) + (x == s.y ? 1u : 0u) + (x == s.z ? 1u : 0u) + (x == s.w ? 1u : 0u);
                    }
                }
                for (int64_t t0 = 0; t0 < m; t0 += M6A_RANKSUM_TILE) {
                    const int cnt = (int)(m - t0 < M6A_RANKSUM_TILE ? m - t0 : M6A_RANKSUM_TILE);
                    ranksum_fill(tile, pb + t0, cnt, lane);
                    if (chunk_has_a) {
                        for (int q = 0; q < (cnt + 3) / 4; q++) {
                            const float4 s = make_float4(tile[4 * q], tile[4 * q + 1], tile[4 * q + 2], tile[4 * q + 3]);   // one 16-byte broadcast
                            ceb += (x == s.x ? 1u : 0u) + (x == s.y ? 1u : 0u) + (x == s.z ? 1u : 0u) + (x == s.w ? 1u : 0u);
                            cgt += (x > s.x ? 1u : 0u) + (x > s.y ? 1u : 0u) + (x > s.z ? 1u : 0u) + (x > s.w ? 1u : 0u);
                        }
                    } else {
                        for (int q = 0; q < (cnt + 3) / 4; q++) {
                            const float4 s = make_float4(tile[4 * q], tile[4 * q + 1], tile[4 * q + 2], tile[4 * q + 3]);   // one 16-byte broadcast
                            ceb += (x == s.x ? 1u : 0u) + (x == s.y ? 1u : 0u) + (x == s.z ? 1u : 0u) + (x == s.w ? 1u : 0u);
                        }
                    }
                }
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

// the launch on the context's stream: a pair per wavefront, four per block; more blocks than are resident, so that ragged bags
// balance over the order in which blocks are handed out
int launch_ranksum(m6a_ctx *c, const RanksumArgs &a)
{
    const unsigned blocks = (unsigned)std::min<int64_t>((a.n_pairs + 3) / 4, (int64_t)c->n_cu * 64);
    hipLaunchKernelGGL(site_ranksum_kernel, dim3(blocks), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    return M6A_OK;
}

}  // namespace

extern "C" int m6a_site_ranksum(m6a_ctx *c, const float *prob_a, const int64_t *off_a, int64_t n_sites_a,
                                const float *prob_b, const int64_t *off_b, int64_t n_sites_b,
                                const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs,
                                int64_t *gt, int64_t *eq, int64_t *tie, double *z)
{
    HintScope hint_scope(c);
    int rc = enter(c);
    if (rc) return rc;
    if (n_sites_a < 0 || n_sites_b < 0 || n_pairs < 0) return fail(c, M6A_EINVAL, "n_sites_a, n_sites_b and n_pairs must be >= 0");
    if (n_pairs == 0) return M6A_OK;
    if ((!pair_a || !pair_b) && (n_pairs != n_sites_a || n_pairs != n_sites_b))
        return fail(c, M6A_EINVAL, "a NULL pair array is the identity and needs n_pairs == n_sites_a == n_sites_b");
    if (!prob_a || !off_a || !prob_b || !off_b || !z) return fail(c, M6A_EINVAL, "null pointer argument");
    HIPCHK(c, hipSetDevice(c->device));
    const int dev = same_side(c, prob_a, {off_a, prob_b, off_b, pair_a, pair_b, gt, eq, tie, z},
                              "prob_a, off_a, prob_b, off_b, pair_a, pair_b, gt, eq, tie, z must be all host or all device pointers");
    if (dev < 0) return dev;
    RanksumArgs a;
    a.n_sites_a = n_sites_a; a.n_sites_b = n_sites_b; a.n_pairs = n_pairs; a.err = c->d_err;
    if (dev) {
        a.prob_a = prob_a; a.prob_b = prob_b; a.off_a = off_a; a.off_b = off_b; a.pair_a = pair_a; a.pair_b = pair_b;
        a.gt = gt; a.eq = eq; a.tie = tie; a.z = z;
        return launch_ranksum(c, a);
    }
    rc = csr_check(c, off_a, n_sites_a);
    if (rc) return rc;
    rc = csr_check(c, off_b, n_sites_b);
    if (rc) return rc;
    for (int64_t k = 0; k < n_pairs; k++) {
        if (pair_a && (pair_a[k] < 0 || pair_a[k] >= n_sites_a)) return fail(c, M6A_EINVAL, "pair_a[%lld] = %lld is outside the %lld sites of the first set", (long long)k, (long long)pair_a[k], (long long)n_sites_a);
        if (pair_b && (pair_b[k] < 0 || pair_b[k] >= n_sites_b)) return fail(c, M6A_EINVAL, "pair_b[%lld] = %lld is outside the %lld sites of the second set", (long long)k, (long long)pair_b[k], (long long)n_sites_b);
    }
    // staged: [0] prob_a [1] off_a [2] prob_b [3] off_b [4] pair_a [5] pair_b in, [6] gt [7] eq [8] tie [9] z out
    DevBuf *s = c->sRank;
    const size_t pb = (size_t)n_pairs * 8;
    HIPCHK(c, stage_in(c, s[0], prob_a, (size_t)off_a[n_sites_a] * 4));
    HIPCHK(c, stage_in(c, s[1], off_a, (size_t)(n_sites_a + 1) * 8));
    HIPCHK(c, stage_in(c, s[2], prob_b, (size_t)off_b[n_sites_b] * 4));
    HIPCHK(c, stage_in(c, s[3], off_b, (size_t)(n_sites_b + 1) * 8));
    if (pair_a) HIPCHK(c, stage_in(c, s[4], pair_a, pb));
    if (pair_b) HIPCHK(c, stage_in(c, s[5], pair_b, pb));
    for (int i = 6; i < 10; i++) HIPCHK(c, s[i].ensure(pb));
    a.prob_a = (const float *)s[0].p; a.off_a = (const int64_t *)s[1].p; a.prob_b = (const float *)s[2].p; a.off_b = (const int64_t *)s[3].p;
    a.pair_a = pair_a ? (const int64_t *)s[4].p : nullptr; a.pair_b = pair_b ? (const int64_t *)s[5].p : nullptr;
    a.gt = gt ? (int64_t *)s[6].p : nullptr; a.eq = eq ? (int64_t *)s[7].p : nullptr; a.tie = tie ? (int64_t *)s[8].p : nullptr;
    a.z = (double *)s[9].p;
    rc = launch_ranksum(c, a);
    if (rc) return rc;
    if (gt) HIPCHK(c, stage_out(c, gt, s[6], pb));
    if (eq) HIPCHK(c, stage_out(c, eq, s[7], pb));
    if (tie) HIPCHK(c, stage_out(c, tie, s[8], pb));
    HIPCHK(c, stage_out(c, z, s[9], pb));
    return sync_and_check(c);
}

// ---- m6a_site_signal_ranksum: the test above on each of the nine columns of X [R][9] ------------------------------------------------
#define M6A_SIGNAL_TILE 256                                   // rows per wavefront in LDS
#define M6A_SIGNAL_STRIDE (M6A_SIGNAL_TILE + 4)               // floats from a column to the next: whole float4s, and 4 c + r (mod 32)
                                                              // is the bank of a transposing write, not r alone -- 9.1 KB per wavefront
#define M6A_SIGNAL_COLS M6A_N_FEATURES

namespace {

struct SignalArgs {
    const float *X_a, *X_b;           // [off_a[n_sites_a]][9], [off_b[n_sites_b]][9]
    const int64_t *off_a, *off_b;     // [n_sites + 1], in rows
    const int64_t *pair_a, *pair_b;   // [n_pairs] or null: the identity
    int64_t n_sites_a, n_sites_b, n_pairs;
    int64_t *gt, *eq, *tie;           // [n_pairs][9], each may be null
    double *z;                        // [n_pairs][9]
    int *err;
};

// cnt <= M6A_SIGNAL_TILE rows [cnt][9] from `rows` into the tile, column c at tile + c * M6A_SIGNAL_STRIDE, every column padded with NaN
// to the next multiple of 4; 9 cnt contiguous dwords, lane l taking dword f0 + l.  Ordered against the reads around it as ranksum_fill is
__device__ __forceinline__ void signal_fill(float *tile, const float *rows, int cnt, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int n_f = cnt * M6A_SIGNAL_COLS;
#pragma unroll 4
    for (int f0 = 0; f0 < n_f; f0 += 64) {                      // uniform
        const int f = f0 + lane;
        if (f < n_f) {
            const int r = f / M6A_SIGNAL_COLS, c = f - r * M6A_SIGNAL_COLS;
            tile[c * M6A_SIGNAL_STRIDE + r] = rows[f];
        }
    }
    const int pad = (4 - (cnt & 3)) & 3;                        // rows cnt .. cnt + pad - 1 of every column: at most 3, below the stride
    if (lane < 3 * M6A_SIGNAL_COLS) {
        const int c = lane / 3, d = lane - 3 * c;
        if (d < pad) tile[c * M6A_SIGNAL_STRIDE + cnt + d] = __builtin_nanf("");
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned signal_count(bool hit) { return hit ? 1u : 0u; }

__global__ __launch_bounds__(256) void site_signal_ranksum_kernel(SignalArgs a)
{
    constexpr int C = M6A_SIGNAL_COLS;
    __shared__ __attribute__((aligned(16))) float lds[4][C * M6A_SIGNAL_STRIDE];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *tile = lds[w];
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t k = (int64_t)blockIdx.x * 4 + w; k < a.n_pairs; k += n_waves) {
        const int64_t ia = a.pair_a ? a.pair_a[k] : k, ib = a.pair_b ? a.pair_b[k] : k;
        bool bad = ia < 0 || ia >= a.n_sites_a || ib < 0 || ib >= a.n_sites_b;
        int64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
        if (!bad) {                                             // nothing is read through an index or an offset before it is checked
            a0 = a.off_a[ia]; a1 = a.off_a[ia + 1];
            b0 = a.off_b[ib]; b1 = a.off_b[ib + 1];
            bad = a0 < 0 || a1 < a0 || a1 > a.off_a[a.n_sites_a] || b0 < 0 || b1 < b0 || b1 > a.off_b[a.n_sites_b];
        }
        const int64_t n = a1 - a0, m = b1 - b0, N = n + m;
        m6a_ranksum::Result r = m6a_ranksum::undefined();      // lane c < 9: column c of the pair
        if (bad) {
            if (lane == 0) atomicExch(a.err, 6);
        } else if (!m6a_ranksum::undefined_sizes(n, m)) {
            const float *pa = a.X_a + a0 * C, *pb = a.X_b + b0 * C;
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
                const bool chunk_has_a = c0 < n;                // uniform: only such a chunk counts the b below its elements
                for (int64_t t0 = 0; t0 < n; t0 += M6A_SIGNAL_TILE) {
                    const int cnt = (int)(n - t0 < M6A_SIGNAL_TILE ? n - t0 : M6A_SIGNAL_TILE);
                    signal_fill(tile, pa + t0 * C, cnt, lane);
                    for (int q = 0; q < (cnt + 3) / 4; q++) {
#pragma unroll
                        for (int c = 0; c < C; c++) {
                            const float4 s = *reinterpret_cast<const float4 *>(tile + c * M6A_SIGNAL_STRIDE + 4 * q);   // one 16-byte broadcast
                            ceq[c] += signal_count(x[c] == s.x) + signal_count(x[c] == s.y) + signal_count(x[c] == s.z) + signal_count(x[c] == s.w);
                        }
                    }
                }
                for (int64_t t0 = 0; t0 < m; t0 += M6A_SIGNAL_TILE) {
                    const int cnt = (int)(m - t0 < M6A_SIGNAL_TILE ? m - t0 : M6A_SIGNAL_TILE);
                    signal_fill(tile, pb + t0 * C, cnt, lane);
                    if (chunk_has_a) {
                        for (int q = 0; q < (cnt + 3) / 4; q++) {
#pragma unroll
                            for (int c = 0; c < C; c++) {
                                const float4 s = *reinterpret_cast<const float4 *>(tile + c * M6A_SIGNAL_STRIDE + 4 * q);
                                ceb[c] += signal_count(x[c] == s.x) + signal_count(x[c] == s.y) + signal_count(x[c] == s.z) + signal_count(x[c] == s.w);
                                cgt[c] += signal_count(x[c] > s.x) + signal_count(x[c] > s.y) + signal_count(x[c] > s.z) + signal_count(x[c] > s.w);
                            }
                        }
                    } else {
                        for (int q = 0; q < (cnt + 3) / 4; q++) {
#pragma unroll
                            for (int c = 0; c < C; c++) {
                                const float4 s = *reinterpret_cast<const float4 *>(tile + c * M6A_SIGNAL_STRIDE + 4 * q);
                                ceb[c] += signal_count(x[c] == s.x) + signal_count(x[c] == s.y) + signal_count(x[c] == s.z) + signal_count(x[c] == s.w);
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
            for (int h = 32; h >= 1; h >>= 1) nan |= (unsigned)__shfl_xor((int)nan, h, 64);
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

// the grid rule of launch_ranksum
int launch_signal_ranksum(m6a_ctx *c, const SignalArgs &a)
{
    const unsigned blocks = (unsigned)std::min<int64_t>((a.n_pairs + 3) / 4, (int64_t)c->n_cu * 64);
    hipLaunchKernelGGL(site_signal_ranksum_kernel, dim3(blocks), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    return M6A_OK;
}

}  // namespace

extern "C" int m6a_site_signal_ranksum(m6a_ctx *c, const float *X_a, const int64_t *off_a, int64_t n_sites_a,
                                       const float *X_b, const int64_t *off_b, int64_t n_sites_b,
                                       const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs,
                                       int64_t *gt, int64_t *eq, int64_t *tie, double *z)
{
    HintScope hint_scope(c);
    int rc = enter(c);
    if (rc) return rc;
    if (n_sites_a < 0 || n_sites_b < 0 || n_pairs < 0) return fail(c, M6A_EINVAL, "n_sites_a, n_sites_b and n_pairs must be >= 0");
    if (n_pairs == 0) return M6A_OK;
    if ((!pair_a || !pair_b) && (n_pairs != n_sites_a || n_pairs != n_sites_b))
        return fail(c, M6A_EINVAL, "a NULL pair array is the identity and needs n_pairs == n_sites_a == n_sites_b");
    if (!X_a || !off_a || !X_b || !off_b || !z) return fail(c, M6A_EINVAL, "null pointer argument");
    HIPCHK(c, hipSetDevice(c->device));
    const int dev = same_side(c, X_a, {off_a, X_b, off_b, pair_a, pair_b, gt, eq, tie, z},
                              "X_a, off_a, X_b, off_b, pair_a, pair_b, gt, eq, tie, z must be all host or all device pointers");
    if (dev < 0) return dev;
    SignalArgs a;
    a.n_sites_a = n_sites_a; a.n_sites_b = n_sites_b; a.n_pairs = n_pairs; a.err = c->d_err;
    if (dev) {
        a.X_a = X_a; a.X_b = X_b; a.off_a = off_a; a.off_b = off_b; a.pair_a = pair_a; a.pair_b = pair_b;
        a.gt = gt; a.eq = eq; a.tie = tie; a.z = z;
        return launch_signal_ranksum(c, a);
    }
    rc = csr_check(c, off_a, n_sites_a);
    if (rc) return rc;
    rc = csr_check(c, off_b, n_sites_b);
    if (rc) return rc;
    for (int64_t k = 0; k < n_pairs; k++) {
        if (pair_a && (pair_a[k] < 0 || pair_a[k] >= n_sites_a)) return fail(c, M6A_EINVAL, "pair_a[%lld] = %lld is outside the %lld sites of the first set", (long long)k, (long long)pair_a[k], (long long)n_sites_a);
        if (pair_b && (pair_b[k] < 0 || pair_b[k] >= n_sites_b)) return fail(c, M6A_EINVAL, "pair_b[%lld] = %lld is outside the %lld sites of the second set", (long long)k, (long long)pair_b[k], (long long)n_sites_b);
    }
    // staged in m6a_site_ranksum's buffers, a row being 36 bytes and a pair's output nine values: [0] X_a [1] off_a [2] X_b [3] off_b
    // [4] pair_a [5] pair_b in, [6] gt [7] eq [8] tie [9] z out
    DevBuf *s = c->sRank;
    const size_t pb = (size_t)n_pairs * 8, ob = pb * M6A_SIGNAL_COLS, row = M6A_SIGNAL_COLS * sizeof(float);
    HIPCHK(c, stage_in(c, s[0], X_a, (size_t)off_a[n_sites_a] * row));
    HIPCHK(c, stage_in(c, s[1], off_a, (size_t)(n_sites_a + 1) * 8));
    HIPCHK(c, stage_in(c, s[2], X_b, (size_t)off_b[n_sites_b] * row));
    HIPCHK(c, stage_in(c, s[3], off_b, (size_t)(n_sites_b + 1) * 8));
    if (pair_a) HIPCHK(c, stage_in(c, s[4], pair_a, pb));
    if (pair_b) HIPCHK(c, stage_in(c, s[5], pair_b, pb));
    for (int i = 6; i < 10; i++) HIPCHK(c, s[i].ensure(ob));
    a.X_a = (const float *)s[0].p; a.off_a = (const int64_t *)s[1].p; a.X_b = (const float *)s[2].p; a.off_b = (const int64_t *)s[3].p;
    a.pair_a = pair_a ? (const int64_t *)s[4].p : nullptr; a.pair_b = pair_b ? (const int64_t *)s[5].p : nullptr;
    a.gt = gt ? (int64_t *)s[6].p : nullptr; a.eq = eq ? (int64_t *)s[7].p : nullptr; a.tie = tie ? (int64_t *)s[8].p : nullptr;
    a.z = (double *)s[9].p;
    rc = launch_signal_ranksum(c, a);
    if (rc) return rc;
    if (gt) HIPCHK(c, stage_out(c, gt, s[6], ob));
    if (eq) HIPCHK(c, stage_out(c, eq, s[7], ob));
    if (tie) HIPCHK(c, stage_out(c, tie, s[8], ob));
    HIPCHK(c, stage_out(c, z, s[9], ob));
    return sync_and_check(c);
}
