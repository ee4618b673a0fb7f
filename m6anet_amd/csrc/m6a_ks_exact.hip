// m6a_ks_exact.hip -- m6a_ks_exact (include/m6a.h): the exact two-sided p-value of the two-sample Kolmogorov-Smirnov statistic, one
// item (n, m, h) per wavefront, a dynamic programme over the (n + 1) x (m + 1) grid of m6a_ks_exact.h in float64.  The walk of the
// wavefronts and the grid rule are m6a_pairs.h's; the caps, the outside test, the band and the cell are m6a_ks_exact.h's, which the host
// compiles too, so kernel and host agree bit for bit.
//   ks_exact_kernel   the shorter bag lies on j (m <= M6A_KS_EXACT_SHORT), the longer on i.  Rows are taken in stripes of 64, stripe s
//                     holding rows 64 s .. 64 s + 63, from the stripe of row n down to stripe 0.  Lane l owns row i0 + l and walks j
//                     downward one step behind lane l + 1: at step t it stands on j = J_hi + 63 - l - t, so all lanes stand on one
//                     anti-diagonal.  v[i][j+1] is the lane's own result of the step before, v[i+1][j] is lane l + 1's, one __shfl_down
//                     of a double per step.  Lane 63 takes row i0 + 64 from the wavefront's boundary row in LDS, where lane 0 of the
//                     stripe before left it; a cell of that row outside the band is 1.0 without a read, so nothing stale is read.
//                     A stripe walks J_lo = j_lo(i0) .. J_hi = j_hi(its last row) only -- the j at which some row of it is inside the
//                     band -- in J_hi - J_lo + 64 steps.  A lane beyond the grid (i > n or j > m) holds 0.0, a lane outside the band
//                     1.0, so the neighbours of the statement come out of the same exchange.  After stripe 0 lane 0 holds v[0][0].
// The cost is about (band cells + 64 rows' skew per stripe) divisions on one wavefront; items differ by five orders of magnitude, so the
// launch hands out many more blocks than are resident.
#pragma clang fp contract(off)
#include "m6a_pairs.h"
#include "m6a_ks_exact.h"

using namespace m6a_detail;

namespace {

struct KsExactArgs {
    const int64_t *n, *m, *h;         // [n_pairs]
    double *p;                        // [n_pairs]
    int64_t n_pairs;                  // the items (named as pair_launch reads it)
};

__global__ __launch_bounds__(256) void ks_exact_kernel(KsExactArgs a)
{
    __shared__ __attribute__((aligned(16))) double lds[M6A_PAIR_WAVES][M6A_KS_EXACT_SHORT + 1];   // 16 KB a wavefront, 64 KB a block
    const int lane = threadIdx.x & 63, w = pair_wave();
    double *edge = lds[w];                                      // edge[j] = v[i0 + 64][j] wherever that cell is inside the band
    const int64_t step = pair_step();
    for (int64_t k = pair_first(w); k < a.n_pairs; k += step) {
        int64_t n = a.n[k], m = a.m[k], h = a.h[k];
        double p;
        if (m6a_kse::undefined(n, m, h)) p = m6a_kse::not_a_number();
        else if (h == 0) p = 1.0;
        else {
            if (m > n) { const int64_t t = n; n = m; m = t; }   // the shorter bag on j: the same bits
            h = m6a_kse::clamp_h(n, m, h);
            double mine = 0.0;
            for (int64_t i0 = n & ~(int64_t)63; i0 >= 0; i0 -= 64) {                           // uniform
                const int64_t top = i0 + 63 < n ? i0 + 63 : n;
                const int64_t J_lo = m6a_kse::j_lo(n, m, h, i0), J_hi = m6a_kse::j_hi(n, m, h, top);
                const int64_t steps = J_hi - J_lo + 64, i = i0 + lane;
                const bool row_in_grid = i <= n, row_above_in_grid = i0 + 64 <= n;
                const double rows_left = (double)(n - i);
                int64_t j = J_hi + 63 - lane;                    // the lane's column at step 0
                int64_t d = m * i - n * j;                       // m i - n j of the lane's cell; + n per step
                // ordered behind the writes of the stripe before (the same wavefront's, in program order)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                mine = J_hi + 1 > m ? 0.0 : 1.0;                 // v[i][J_hi + 1]: beyond the grid, or outside the band of every row of the stripe
                for (int64_t t = 0; t < steps; t++, j--, d += n) {
                    double below = __shfl_down(mine, 1, 64);     // lane l + 1's cell of the step before: (i + 1, j)
                    if (lane == 63) {
                        below = row_above_in_grid ? 1.0 : 0.0;
                        if (row_above_in_grid && j >= 0 && j <= m && !m6a_kse::outside(d + m, h)) below = edge[j];
                    }
                    double v;
                    if (!row_in_grid || j > m) v = 0.0;          // beyond the grid
                    else if (j < 0 || m6a_kse::outside(d, h)) v = 1.0;   // (j < 0: past the row's end, read by no one)
                    else if (i == n && j == m) v = 0.0;
                    else v = m6a_kse::cell(rows_left, below, (double)(m - j), mine, (double)(n + m - i - j));
                    mine = v;
                    if (lane == 0 && j >= 0 && j <= m) edge[j] = v;   // row i0: the boundary of the stripe below
                }
            }
            p = mine;                                            // lane 0: v[0][0], the last step of stripe 0
        }
        if (lane == 0) a.p[k] = p;
    }
}

}  // namespace

extern "C" int m6a_ks_exact(m6a_ctx *c, const int64_t *n, const int64_t *m, const int64_t *h, int64_t count, double *p)
{
    HintScope hint_scope(c);
    int rc = enter(c);
    if (rc) return rc;
    if (count < 0) return fail(c, M6A_EINVAL, "count must be >= 0");
    if (count == 0) return M6A_OK;
    if (!n || !m || !h || !p) return fail(c, M6A_EINVAL, "null pointer argument");
    HIPCHK(c, hipSetDevice(c->device));
    const int dev = same_side(c, n, {m, h, p}, "n, m, h and p must be all host or all device pointers");
    if (dev < 0) return dev;
    if (dev) return pair_launch(c, ks_exact_kernel, KsExactArgs{n, m, h, p, count});
    DevBuf *s = c->sRank;                                       // as pair_call stages: [0] n [1] m [2] h in, [6] p out
    const size_t bytes = (size_t)count * 8;
    HIPCHK(c, stage_in(c, s[0], n, bytes));
    HIPCHK(c, stage_in(c, s[1], m, bytes));
    HIPCHK(c, stage_in(c, s[2], h, bytes));
    HIPCHK(c, s[6].ensure(bytes));
    rc = pair_launch(c, ks_exact_kernel, KsExactArgs{(const int64_t *)s[0].p, (const int64_t *)s[1].p, (const int64_t *)s[2].p, (double *)s[6].p, count});
    if (rc) return rc;
    HIPCHK(c, stage_out(c, p, s[6], bytes));
    return sync_and_check(c);
}
