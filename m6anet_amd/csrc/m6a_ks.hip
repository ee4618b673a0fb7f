// m6a_ks.hip -- m6a_site_ks and m6a_site_signal_ks (include/m6a.h): the two integers of the two-sample Kolmogorov-Smirnov statistic and
// the two medians of pairs of sites, one site from each of two sets.  The counting is all-pairs and exact in integers, as in
// m6a_ranksum.hip, whose scheme this is; the medians' closing line is m6a_ks.h's, which the host compiles too.
//   site_ks_kernel         a wavefront per pair.  The pooled sample a ++ b (N = n + m reads) is walked in chunks of 64: lane l owns pooled
//                          element c0 + l.  For every chunk both bags stream through the wavefront's LDS tile (M6A_KS_TILE floats, padded
//                          to whole float4s with NaN, which compares false), read back as float4 broadcasts.  A lane counts s <= x
//                          against both bags -- A(x) and B(x) -- and s < x against its own bag, the latter only in chunks that hold
//                          elements of that bag (uniform).  At the end of its chunk a lane's element is completely counted: it folds
//                          t = m A - n B and -t into two running 64-bit maxima, and keeps its value as a middle of its bag where
//                          lt <= k < le for k = (s - 1) / 2 or s / 2.  No sum crosses a chunk and no float is added before the closing
//                          line; two integer max butterflies and four picks among the qualifying lanes (whose values compare equal)
//                          close the pair.
//   site_signal_ks_kernel  the same on each of the nine columns of X [R][9]: lane l owns pooled ROW c0 + l with its nine values in
//                          registers, a tile of M6A_KS_SIGNAL_TILE rows is loaded once per (chunk, tile) and kept column-major in LDS
//                          (the layout of m6a_ranksum.hip's signal_fill, copied here since that unit's helpers are its own), 27 32-bit
//                          counters per chunk, 18 64-bit maxima and 36 median candidates per lane; lanes 0..8 close one column each.
// The cost is N^2 compares per pair and column on one wavefront, as for the rank-sum: bags of tens to a few thousand reads.
#pragma clang fp contract(off)
#include "m6a_ctx.h"
#include "m6a_ks.h"

using namespace m6a_detail;

#define M6A_KS_TILE 256                                       // floats per wavefront in LDS: 1 KB, 4 KB per block
#define M6A_KS_SIGNAL_TILE 256                                // rows per wavefront in LDS
#define M6A_KS_SIGNAL_STRIDE (M6A_KS_SIGNAL_TILE + 4)         // floats from a column to the next: whole float4s; 9.1 KB per wavefront
#define M6A_KS_COLS M6A_N_FEATURES

namespace {

struct KsArgs {
    const float *v_a, *v_b;           // [off_a[n_sites_a]], [off_b[n_sites_b]] values (m6a_site_ks) or rows of nine (m6a_site_signal_ks)
    const int64_t *off_a, *off_b;     // [n_sites + 1]
    const int64_t *pair_a, *pair_b;   // [n_pairs] or null: the identity
    int64_t n_sites_a, n_sites_b, n_pairs;
    int64_t *d_pos, *d_neg;           // [n_pairs] or [n_pairs][9]
    double *med_a, *med_b;            // the same shape, each may be null
    int *err;
};

// the pair's two bags as rows [a0, a1) and [b0, b1), or bad: nothing is read through an index or an offset before it is checked
__device__ __forceinline__ bool ks_pair(const KsArgs &a, int64_t k, int64_t &a0, int64_t &a1, int64_t &b0, int64_t &b1)
{
    const int64_t ia = a.pair_a ? a.pair_a[k] : k, ib = a.pair_b ? a.pair_b[k] : k;
    a0 = a1 = b0 = b1 = 0;
    if (ia < 0 || ia >= a.n_sites_a || ib < 0 || ib >= a.n_sites_b) return false;
    a0 = a.off_a[ia]; a1 = a.off_a[ia + 1];
    b0 = a.off_b[ib]; b1 = a.off_b[ib + 1];
    return !(a0 < 0 || a1 < a0 || a1 > a.off_a[a.n_sites_a] || b0 < 0 || b1 < b0 || b1 > a.off_b[a.n_sites_b]);
}

// cnt <= M6A_KS_TILE floats from p into the tile, NaN up to the next multiple of 4; ordered against the reads around it
__device__ __forceinline__ void ks_fill(float *tile, const float *p, int cnt, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < M6A_KS_TILE / 64; k++) {
        if (k * 64 >= cnt) break;                               // uniform
        const int j = k * 64 + lane;
        tile[j] = j < cnt ? p[j] : __builtin_nanf("");
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ long long ks_wave_max(long long v)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        const long long o = __shfl_xor(v, h, 64);
        v = o > v ? o : v;
    }
    return v;
}

// the value of the first lane that holds a candidate (not NaN); every candidate of a defined bag compares equal to it
__device__ __forceinline__ float ks_pick(float cand)
{
    const unsigned long long has = __ballot(cand == cand);
    return __shfl(cand, has ? __builtin_ctzll(has) : 0, 64);
}

__device__ __forceinline__ unsigned ks_one(bool hit) { return hit ? 1u : 0u; }

// one bag through the tile against every lane's x: le += #{s <= x}; LT: lt += #{s < xl}, xl being x in the lanes whose element is of
// this bag and -inf, which nothing is below, in the others
template <bool LT>
__device__ __forceinline__ void ks_stream(float *tile, const float *p, int64_t len, int lane, float x, float xl, unsigned &le, unsigned &lt)
{
    for (int64_t t0 = 0; t0 < len; t0 += M6A_KS_TILE) {
        const int cnt = (int)(len - t0 < M6A_KS_TILE ? len - t0 : M6A_KS_TILE);
        ks_fill(tile, p + t0, cnt, lane);
        for (int q = 0; q < (cnt + 3) / 4; q++) {
            const float4 s = make_float4(tile[4 * q], tile[4 * q + 1], tile[4 * q + 2], tile[4 * q + 3]);   // one 16-byte broadcast
            le += ks_one(s.x <= x) + ks_one(s.y <= x) + ks_one(s.z <= x) + ks_one(s.w <= x);
            if (LT) lt += ks_one(s.x < xl) + ks_one(s.y < xl) + ks_one(s.z < xl) + ks_one(s.w < xl);
        }
    }
}

__global__ __launch_bounds__(256) void site_ks_kernel(KsArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[4][M6A_KS_TILE];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *tile = lds[w];
    const float none = __builtin_nanf(""), below_all = -__builtin_inff();
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t k = (int64_t)blockIdx.x * 4 + w; k < a.n_pairs; k += n_waves) {
        int64_t a0, a1, b0, b1;
        const bool bad = !ks_pair(a, k, a0, a1, b0, b1);
        const int64_t n = a1 - a0, m = b1 - b0, N = n + m;
        m6a_ks::Result r = m6a_ks::undefined();
        if (bad) {
            if (lane == 0) atomicExch(a.err, 7);
        } else if (!m6a_ranksum::undefined_sizes(n, m)) {
            const float *pa = a.v_a + a0, *pb = a.v_b + b0;
            long long d_pos = 0, d_neg = 0;                     // both are >= 0: t = 0 at the largest pooled value
            float lo_a = none, hi_a = none, lo_b = none, hi_b = none;
            bool nan = false;
            for (int64_t c0 = 0; c0 < N; c0 += 64) {
                const int64_t i = c0 + lane;
                const bool own = i < N, of_a = i < n, of_b = own && !of_a;
                const float x = own ? (of_a ? pa[i] : pb[i - n]) : none;
                nan = nan || (own && x != x);
                unsigned le_a = 0, le_b = 0, lt = 0;            // lt: of the lane's own bag
                if (c0 < n) ks_stream<true>(tile, pa, n, lane, x, of_a ? x : below_all, le_a, lt);      // uniform: the chunk holds elements of a
                else ks_stream<false>(tile, pa, n, lane, x, x, le_a, lt);
                if (c0 + 64 > n) ks_stream<true>(tile, pb, m, lane, x, of_b ? x : below_all, le_b, lt); // uniform: ... of b
                else ks_stream<false>(tile, pb, m, lane, x, x, le_b, lt);
                if (own) {                                      // this element is completely counted
                    const long long t = (long long)m * le_a - (long long)n * le_b;
                    d_pos = t > d_pos ? t : d_pos;
                    d_neg = -t > d_neg ? -t : d_neg;
                    const unsigned le = of_a ? le_a : le_b, s = (unsigned)(of_a ? n : m), k_lo = (s - 1) / 2, k_hi = s / 2;
                    const bool is_lo = lt <= k_lo && k_lo < le, is_hi = lt <= k_hi && k_hi < le;
                    if (is_lo && of_a) lo_a = x;
                    if (is_hi && of_a) hi_a = x;
                    if (is_lo && of_b) lo_b = x;
                    if (is_hi && of_b) hi_b = x;
                }
            }
            d_pos = ks_wave_max(d_pos);
            d_neg = ks_wave_max(d_neg);
            lo_a = ks_pick(lo_a); hi_a = ks_pick(hi_a); lo_b = ks_pick(lo_b); hi_b = ks_pick(hi_b);
            if (__ballot(nan) == 0ull) r = {(int64_t)d_pos, (int64_t)d_neg, m6a_ks::median(lo_a, hi_a), m6a_ks::median(lo_b, hi_b)};
        }
        if (lane == 0) {
            a.d_pos[k] = r.d_pos;
            a.d_neg[k] = r.d_neg;
            if (a.med_a) a.med_a[k] = r.med_a;
            if (a.med_b) a.med_b[k] = r.med_b;
        }
    }
}

// ---- m6a_site_signal_ks: the same on each of the nine columns of X [R][9] -------------------------------------------------------------

// cnt <= M6A_KS_SIGNAL_TILE rows [cnt][9] from `rows` into the tile, column c at tile + c * M6A_KS_SIGNAL_STRIDE, every column padded
// with NaN to the next multiple of 4; 9 cnt contiguous dwords, lane l taking dword f0 + l (m6a_ranksum.hip's signal_fill)
__device__ __forceinline__ void ks_signal_fill(float *tile, const float *rows, int cnt, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int n_f = cnt * M6A_KS_COLS;
#pragma unroll 4
    for (int f0 = 0; f0 < n_f; f0 += 64) {                      // uniform
        const int f = f0 + lane;
        if (f < n_f) {
            const int r = f / M6A_KS_COLS, c = f - r * M6A_KS_COLS;
            tile[c * M6A_KS_SIGNAL_STRIDE + r] = rows[f];
        }
    }
    const int pad = (4 - (cnt & 3)) & 3;                        // rows cnt .. cnt + pad - 1 of every column: at most 3, below the stride
    if (lane < 3 * M6A_KS_COLS) {
        const int c = lane / 3, d = lane - 3 * c;
        if (d < pad) tile[c * M6A_KS_SIGNAL_STRIDE + cnt + d] = __builtin_nanf("");
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ks_stream on rows: every column of one bag against the lane's row
template <bool LT>
__device__ __forceinline__ void ks_signal_stream(float *tile, const float *p, int64_t len, int lane, const float (&x)[M6A_KS_COLS], bool mine,
                                                 unsigned (&le)[M6A_KS_COLS], unsigned (&lt)[M6A_KS_COLS])
{
    constexpr int C = M6A_KS_COLS;
    float xl[C];
#pragma unroll
    for (int c = 0; c < C; c++) xl[c] = mine ? x[c] : -__builtin_inff();
    for (int64_t t0 = 0; t0 < len; t0 += M6A_KS_SIGNAL_TILE) {
        const int cnt = (int)(len - t0 < M6A_KS_SIGNAL_TILE ? len - t0 : M6A_KS_SIGNAL_TILE);
        ks_signal_fill(tile, p + t0 * C, cnt, lane);
        for (int q = 0; q < (cnt + 3) / 4; q++) {
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float4 s = *reinterpret_cast<const float4 *>(tile + c * M6A_KS_SIGNAL_STRIDE + 4 * q);   // one 16-byte broadcast
                le[c] += ks_one(s.x <= x[c]) + ks_one(s.y <= x[c]) + ks_one(s.z <= x[c]) + ks_one(s.w <= x[c]);
                if (LT) lt[c] += ks_one(s.x < xl[c]) + ks_one(s.y < xl[c]) + ks_one(s.z < xl[c]) + ks_one(s.w < xl[c]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void site_signal_ks_kernel(KsArgs a)
{
    constexpr int C = M6A_KS_COLS;
    __shared__ __attribute__((aligned(16))) float lds[4][C * M6A_KS_SIGNAL_STRIDE];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *tile = lds[w];
    const float none = __builtin_nanf("");
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t k = (int64_t)blockIdx.x * 4 + w; k < a.n_pairs; k += n_waves) {
        int64_t a0, a1, b0, b1;
        const bool bad = !ks_pair(a, k, a0, a1, b0, b1);
        const int64_t n = a1 - a0, m = b1 - b0, N = n + m;
        m6a_ks::Result r = m6a_ks::undefined();                // lane c < 9: column c of the pair
        if (bad) {
            if (lane == 0) atomicExch(a.err, 8);
        } else if (!m6a_ranksum::undefined_sizes(n, m)) {
            const float *pa = a.v_a + a0 * C, *pb = a.v_b + b0 * C;
            long long d_pos[C], d_neg[C];
            float lo_a[C], hi_a[C], lo_b[C], hi_b[C];
#pragma unroll
            for (int c = 0; c < C; c++) {
                d_pos[c] = d_neg[c] = 0;
                lo_a[c] = hi_a[c] = lo_b[c] = hi_b[c] = none;
            }
            unsigned nan = 0;                                   // bit c: a NaN in column c of a row this lane owned
            for (int64_t c0 = 0; c0 < N; c0 += 64) {
                const int64_t i = c0 + lane;
                const bool own = i < N, of_a = i < n, of_b = own && !of_a;
                const float *row = !own ? pa : of_a ? pa + i * C : pb + (i - n) * C;   // (pa: a row that exists, read by no one)
                float x[C];
                unsigned le_a[C], le_b[C], lt[C];
#pragma unroll
                for (int c = 0; c < C; c++) {
                    x[c] = own ? row[c] : none;
                    if (own && x[c] != x[c]) nan |= 1u << c;
                    le_a[c] = le_b[c] = lt[c] = 0;
                }
                if (c0 < n) ks_signal_stream<true>(tile, pa, n, lane, x, of_a, le_a, lt);               // uniform: the chunk holds rows of a
                else ks_signal_stream<false>(tile, pa, n, lane, x, false, le_a, lt);
                if (c0 + 64 > n) ks_signal_stream<true>(tile, pb, m, lane, x, of_b, le_b, lt);          // uniform: ... of b
                else ks_signal_stream<false>(tile, pb, m, lane, x, false, le_b, lt);
                if (own) {                                      // this row is completely counted
                    const unsigned s = (unsigned)(of_a ? n : m), k_lo = (s - 1) / 2, k_hi = s / 2;
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        const long long t = (long long)m * le_a[c] - (long long)n * le_b[c];
                        d_pos[c] = t > d_pos[c] ? t : d_pos[c];
                        d_neg[c] = -t > d_neg[c] ? -t : d_neg[c];
                        const unsigned le = of_a ? le_a[c] : le_b[c];
                        const bool is_lo = lt[c] <= k_lo && k_lo < le, is_hi = lt[c] <= k_hi && k_hi < le;
                        if (is_lo && of_a) lo_a[c] = x[c];
                        if (is_hi && of_a) hi_a[c] = x[c];
                        if (is_lo && of_b) lo_b[c] = x[c];
                        if (is_hi && of_b) hi_b[c] = x[c];
                    }
                }
            }
            long long p = 0, g = 0;
            float la = none, ha = none, lb = none, hb = none;
#pragma unroll
            for (int c = 0; c < C; c++) {                       // every lane holds the pair's results; lane c keeps column c's
                const long long sp = ks_wave_max(d_pos[c]), sg = ks_wave_max(d_neg[c]);
                const float vla = ks_pick(lo_a[c]), vha = ks_pick(hi_a[c]), vlb = ks_pick(lo_b[c]), vhb = ks_pick(hi_b[c]);
                if (lane == c) { p = sp; g = sg; la = vla; ha = vha; lb = vlb; hb = vhb; }
            }
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1) nan |= (unsigned)__shfl_xor((int)nan, h, 64);
            if (lane < C && !((nan >> lane) & 1u)) r = {(int64_t)p, (int64_t)g, m6a_ks::median(la, ha), m6a_ks::median(lb, hb)};
        }
        if (lane < C) {
            const int64_t at = k * C + lane;
            a.d_pos[at] = r.d_pos;
            a.d_neg[at] = r.d_neg;
            if (a.med_a) a.med_a[at] = r.med_a;
            if (a.med_b) a.med_b[at] = r.med_b;
        }
    }
}

// the launch on the context's stream, by the grid rule of m6a_ranksum.hip's launch_ranksum: a pair per wavefront, four per block; more
// blocks than are resident, so that ragged bags balance over the order in which blocks are handed out
int launch_ks(m6a_ctx *c, const KsArgs &a, int cols)
{
    const unsigned blocks = (unsigned)std::min<int64_t>((a.n_pairs + 3) / 4, (int64_t)c->n_cu * 64);
    if (cols == 1) hipLaunchKernelGGL(site_ks_kernel, dim3(blocks), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(site_signal_ks_kernel, dim3(blocks), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    return M6A_OK;
}

// both entry points: a bag's element is `cols` float32 (1: a value, 9: a row of X) and a pair's output `cols` values
int site_ks_call(m6a_ctx *c, int cols, const float *v_a, const int64_t *off_a, int64_t n_sites_a, const float *v_b, const int64_t *off_b,
                 int64_t n_sites_b, const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs, int64_t *d_pos, int64_t *d_neg,
                 double *med_a, double *med_b)
{
    HintScope hint_scope(c);
    int rc = enter(c);
    if (rc) return rc;
    if (n_sites_a < 0 || n_sites_b < 0 || n_pairs < 0) return fail(c, M6A_EINVAL, "n_sites_a, n_sites_b and n_pairs must be >= 0");
    if (n_pairs == 0) return M6A_OK;
    if ((!pair_a || !pair_b) && (n_pairs != n_sites_a || n_pairs != n_sites_b))
        return fail(c, M6A_EINVAL, "a NULL pair array is the identity and needs n_pairs == n_sites_a == n_sites_b");
    if (!v_a || !off_a || !v_b || !off_b || !d_pos || !d_neg) return fail(c, M6A_EINVAL, "null pointer argument");
    HIPCHK(c, hipSetDevice(c->device));
    const int dev = same_side(c, v_a, {off_a, v_b, off_b, pair_a, pair_b, d_pos, d_neg, med_a, med_b},
                              "the two sets, off_a, off_b, pair_a, pair_b, d_pos, d_neg, med_a, med_b must be all host or all device pointers");
    if (dev < 0) return dev;
    KsArgs a;
    a.n_sites_a = n_sites_a; a.n_sites_b = n_sites_b; a.n_pairs = n_pairs; a.err = c->d_err;
    if (dev) {
        a.v_a = v_a; a.v_b = v_b; a.off_a = off_a; a.off_b = off_b; a.pair_a = pair_a; a.pair_b = pair_b;
        a.d_pos = d_pos; a.d_neg = d_neg; a.med_a = med_a; a.med_b = med_b;
        return launch_ks(c, a, cols);
    }
    rc = csr_check(c, off_a, n_sites_a);
    if (rc) return rc;
    rc = csr_check(c, off_b, n_sites_b);
    if (rc) return rc;
    for (int64_t k = 0; k < n_pairs; k++) {
        if (pair_a && (pair_a[k] < 0 || pair_a[k] >= n_sites_a)) return fail(c, M6A_EINVAL, "pair_a[%lld] = %lld is outside the %lld sites of the first set", (long long)k, (long long)pair_a[k], (long long)n_sites_a);
        if (pair_b && (pair_b[k] < 0 || pair_b[k] >= n_sites_b)) return fail(c, M6A_EINVAL, "pair_b[%lld] = %lld is outside the %lld sites of the second set", (long long)k, (long long)pair_b[k], (long long)n_sites_b);
    }
    // staged in m6a_site_ranksum's buffers (the calls are synchronous, one at a time): [0] v_a [1] off_a [2] v_b [3] off_b [4] pair_a
    // [5] pair_b in, [6] d_pos [7] d_neg [8] med_a [9] med_b out
    DevBuf *s = c->sRank;
    const size_t pb = (size_t)n_pairs * 8, ob = pb * (size_t)cols, el = (size_t)cols * sizeof(float);
    HIPCHK(c, stage_in(c, s[0], v_a, (size_t)off_a[n_sites_a] * el));
    HIPCHK(c, stage_in(c, s[1], off_a, (size_t)(n_sites_a + 1) * 8));
    HIPCHK(c, stage_in(c, s[2], v_b, (size_t)off_b[n_sites_b] * el));
    HIPCHK(c, stage_in(c, s[3], off_b, (size_t)(n_sites_b + 1) * 8));
    if (pair_a) HIPCHK(c, stage_in(c, s[4], pair_a, pb));
    if (pair_b) HIPCHK(c, stage_in(c, s[5], pair_b, pb));
    for (int i = 6; i < 10; i++) HIPCHK(c, s[i].ensure(ob));
    a.v_a = (const float *)s[0].p; a.off_a = (const int64_t *)s[1].p; a.v_b = (const float *)s[2].p; a.off_b = (const int64_t *)s[3].p;
    a.pair_a = pair_a ? (const int64_t *)s[4].p : nullptr; a.pair_b = pair_b ? (const int64_t *)s[5].p : nullptr;
    a.d_pos = (int64_t *)s[6].p; a.d_neg = (int64_t *)s[7].p;
    a.med_a = med_a ? (double *)s[8].p : nullptr; a.med_b = med_b ? (double *)s[9].p : nullptr;
    rc = launch_ks(c, a, cols);
    if (rc) return rc;
    HIPCHK(c, stage_out(c, d_pos, s[6], ob));
    HIPCHK(c, stage_out(c, d_neg, s[7], ob));
    if (med_a) HIPCHK(c, stage_out(c, med_a, s[8], ob));
    if (med_b) HIPCHK(c, stage_out(c, med_b, s[9], ob));
    return sync_and_check(c);
}

}  // namespace

extern "C" int m6a_site_ks(m6a_ctx *c, const float *prob_a, const int64_t *off_a, int64_t n_sites_a,
                           const float *prob_b, const int64_t *off_b, int64_t n_sites_b,
                           const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs,
                           int64_t *d_pos, int64_t *d_neg, double *med_a, double *med_b)
{
    return site_ks_call(c, 1, prob_a, off_a, n_sites_a, prob_b, off_b, n_sites_b, pair_a, pair_b, n_pairs, d_pos, d_neg, med_a, med_b);
}

extern "C" int m6a_site_signal_ks(m6a_ctx *c, const float *X_a, const int64_t *off_a, int64_t n_sites_a,
                                  const float *X_b, const int64_t *off_b, int64_t n_sites_b,
                                  const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs,
                                  int64_t *d_pos, int64_t *d_neg, double *med_a, double *med_b)
{
    return site_ks_call(c, M6A_KS_COLS, X_a, off_a, n_sites_a, X_b, off_b, n_sites_b, pair_a, pair_b, n_pairs, d_pos, d_neg, med_a, med_b);
}
