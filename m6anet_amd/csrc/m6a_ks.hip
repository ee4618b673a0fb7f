// m6a_ks.hip -- m6a_site_ks and m6a_site_signal_ks (include/m6a.h): the two integers of the two-sample Kolmogorov-Smirnov statistic and
// the two medians of pairs of sites, one site from each of two sets.  The counting is all-pairs and exact in integers, as in
// m6a_ranksum.hip; the scheme -- the pair header, the tile fills, the walk and the launch, the entry point -- is m6a_pairs.h's, shared with
// that unit; the medians' closing line is m6a_ks.h's, which the host compiles too.
//   site_ks_kernel         a wavefront per pair.  The pooled sample a ++ b (N = n + m reads) is walked in chunks of 64: lane l owns pooled
//                          element c0 + l.  For every chunk both bags stream through the wavefront's LDS tile (M6A_PAIR_TILE floats, padded
//                          to whole float4s with NaN, which compares false), read back as float4 broadcasts.  A lane counts s <= x
//                          against both bags -- A(x) and B(x) -- and s < x against its own bag, the latter only in chunks that hold
//                          elements of that bag (uniform).  At the end of its chunk a lane's element is completely counted: it folds
//                          t = m A - n B and -t into two running 64-bit maxima, and keeps its value as a middle of its bag where
//                          lt <= k < le for k = (s - 1) / 2 or s / 2.  No sum crosses a chunk and no float is added before the closing
//                          line; two integer max butterflies and four picks among the qualifying lanes (whose values compare equal)
//                          close the pair.
//   site_signal_ks_kernel  the same on each of the nine columns of X [R][9]: lane l owns pooled ROW c0 + l with its nine values in
//                          registers, a tile of M6A_PAIR_TILE rows is loaded once per (chunk, tile) and kept column-major in LDS
//                          (pair_fill_rows), 27 32-bit counters per chunk, 18 64-bit maxima and 36 median candidates per lane; lanes
//                          0..8 close one column each.
// The cost is N^2 compares per pair and column on one wavefront, as for the rank-sum: bags of tens to a few thousand reads.
#pragma clang fp contract(off)
#include "m6a_pairs.h"
#include "m6a_ks.h"

using namespace m6a_detail;

namespace {

struct KsArgs : PairsIn {
    int64_t *d_pos, *d_neg;           // [n_pairs] or [n_pairs][9]
    double *med_a, *med_b;            // the same shape, each may be null
    int *err;
};

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

// one bag through the tile against every lane's x: le += #{s <= x}; LT: lt += #{s < xl}, xl being x in the lanes whose element is of
// this bag and -inf, which nothing is below, in the others
template <bool LT>
__device__ __forceinline__ void ks_stream(float *tile, const float *p, int64_t len, int lane, float x, float xl, unsigned &le, unsigned &lt)
{
    for (int64_t t0 = 0; t0 < len; t0 += M6A_PAIR_TILE) {
        const int cnt = (int)(len - t0 < M6A_PAIR_TILE ? len - t0 : M6A_PAIR_TILE);
        pair_fill(tile, p + t0, cnt, lane);
        for (int q = 0; q < (cnt + 3) / 4; q++) {
            const float4 s = make_float4(tile[4 * q], tile[4 * q + 1], tile[4 * q + 2], tile[4 * q + 3]);   // one 16-byte broadcast
            le += pair_one(s.x <= x) + pair_one(s.y <= x) + pair_one(s.z <= x) + pair_one(s.w <= x);
            if (LT) lt += pair_one(s.x < xl) + pair_one(s.y < xl) + pair_one(s.z < xl) + pair_one(s.w < xl);
        }
    }
}

__global__ __launch_bounds__(256) void site_ks_kernel(KsArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[M6A_PAIR_WAVES][M6A_PAIR_TILE];
    const int lane = threadIdx.x & 63, w = pair_wave();
    float *tile = lds[w];
    const float none = __builtin_nanf(""), below_all = -__builtin_inff();
    const int64_t step = pair_step();
    for (int64_t k = pair_first(w); k < a.n_pairs; k += step) {
        int64_t a0, a1, b0, b1;
        const bool bad = !pair_bags(a, k, a0, a1, b0, b1);
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

// ks_stream on rows: every column of one bag against the lane's row
template <bool LT>
__device__ __forceinline__ void ks_signal_stream(float *tile, const float *p, int64_t len, int lane, const float (&x)[M6A_PAIR_COLS], bool mine,
                                                 unsigned (&le)[M6A_PAIR_COLS], unsigned (&lt)[M6A_PAIR_COLS])
{
    constexpr int C = M6A_PAIR_COLS;
    float xl[C];
#pragma unroll
    for (int c = 0; c < C; c++) xl[c] = mine ? x[c] : -__builtin_inff();
    for (int64_t t0 = 0; t0 < len; t0 += M6A_PAIR_TILE) {
        const int cnt = (int)(len - t0 < M6A_PAIR_TILE ? len - t0 : M6A_PAIR_TILE);
        pair_fill_rows(tile, p + t0 * C, cnt, lane);
        for (int q = 0; q < (cnt + 3) / 4; q++) {
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float4 s = *reinterpret_cast<const float4 *>(tile + c * M6A_PAIR_STRIDE + 4 * q);   // one 16-byte broadcast
                le[c] += pair_one(s.x <= x[c]) + pair_one(s.y <= x[c]) + pair_one(s.z <= x[c]) + pair_one(s.w <= x[c]);
                if (LT) lt[c] += pair_one(s.x < xl[c]) + pair_one(s.y < xl[c]) + pair_one(s.z < xl[c]) + pair_one(s.w < xl[c]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void site_signal_ks_kernel(KsArgs a)
{
    constexpr int C = M6A_PAIR_COLS;
    __shared__ __attribute__((aligned(16))) float lds[M6A_PAIR_WAVES][C * M6A_PAIR_STRIDE];
    const int lane = threadIdx.x & 63, w = pair_wave();
    float *tile = lds[w];
    const float none = __builtin_nanf("");
    const int64_t step = pair_step();
    for (int64_t k = pair_first(w); k < a.n_pairs; k += step) {
        int64_t a0, a1, b0, b1;
        const bool bad = !pair_bags(a, k, a0, a1, b0, b1);
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
            for (int h = 32; h >= 1; h >>= 1) nan |= (unsigned)__shfl_xor((int)nan, h, 64);   // (as a helper in m6a_pairs.h it moves this build)
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

// both entry points: d_pos and d_neg are required, the medians are not
int site_ks_call(m6a_ctx *c, int cols, const float *v_a, const int64_t *off_a, int64_t n_sites_a, const float *v_b, const int64_t *off_b,
                 int64_t n_sites_b, const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs, int64_t *d_pos, int64_t *d_neg,
                 double *med_a, double *med_b)
{
    return pair_call(c, cols, v_a, off_a, n_sites_a, v_b, off_b, n_sites_b, pair_a, pair_b, n_pairs, {d_pos, d_neg, med_a, med_b},
                     {true, true, false, false},
                     "the two sets, off_a, off_b, pair_a, pair_b, d_pos, d_neg, med_a, med_b must be all host or all device pointers",
                     [c, cols](const PairsIn &in, void *const *o) {
                         return pair_launch(c, cols == 1 ? site_ks_kernel : site_signal_ks_kernel,
                                            KsArgs{in, (int64_t *)o[0], (int64_t *)o[1], (double *)o[2], (double *)o[3], c->d_err});
                     });
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
    return site_ks_call(c, M6A_PAIR_COLS, X_a, off_a, n_sites_a, X_b, off_b, n_sites_b, pair_a, pair_b, n_pairs, d_pos, d_neg, med_a, med_b);
}
