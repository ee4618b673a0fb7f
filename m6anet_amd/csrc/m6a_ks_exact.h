// m6a_ks_exact.h -- the exact two-sample Kolmogorov-Smirnov p-value (include/m6a.h: m6a_ks_exact), the part both sides share.  Plain C++
// marked for host and device, as m6a_ks.h is: m6a_ks_exact.hip compiles the caps, the outside test, the band and the cell for gfx950
// behind its kernel, m6a_io.cpp compiles all of it for the CPU (m6a_io_ks_exact), and tests/ks_exact_core_main.cpp runs it as a program
// of its own under ASan and UBSan.  The p-value is a recurrence over the cells (i, j) of an (n + 1) x (m + 1) grid whose every cell is two
// IEEE products, one sum and one division, each rounded on its own and none re-ordered (the builds pass -ffp-contract=off), so any
// schedule that hands a cell its two neighbours gives the same bits.  The recurrence is symmetric under swapping the two bags and IEEE
// addition commutes, so either bag may lie on either axis.
//   p_value()   one item on the host: the shorter bag on j, one row of m + 2 doubles updated in place from row n down to row 0, only the
//               cells inside the band |m i - n j| < h computed -- O(n + cells inside the band).
#ifndef M6A_KS_EXACT_H
#define M6A_KS_EXACT_H
#include "m6a_ranksum.h"

// (include/m6a.h has the same two lines; this header is also compiled without it)
#define M6A_KS_EXACT_SHORT 2047                               // min(n, m) above this: undefined (the boundary row of min + 1 doubles a wavefront keeps in LDS)
#define M6A_KS_EXACT_CELLS 100000000                          // n m above this: undefined (scipy's own 10 000 x 10 000)

namespace m6a_kse {

M6A_HD inline double not_a_number()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_nan("");
#else
    return NAN;
#endif
}

// an empty bag, the undefined pair of the KS kernels (d_pos = d_neg = -1), or a grid past either cap; no product is formed before its
// factors are known to be small
M6A_HD inline bool undefined(int64_t n, int64_t m, int64_t h)
{
    if (n < 1 || m < 1 || h < 0) return true;
    const int64_t lo = n < m ? n : m, hi = n < m ? m : n;
    return lo > M6A_KS_EXACT_SHORT || hi > M6A_KS_EXACT_CELLS || lo * hi > M6A_KS_EXACT_CELLS;
}

// h as the recurrence sees it: every h above n m leaves every cell inside, as n m + 1 does (so m i + h stays far inside int64)
M6A_HD inline int64_t clamp_h(int64_t n, int64_t m, int64_t h) { return h > n * m ? n * m + 1 : h; }

// d = m i - n j of a cell: the cell is outside, v = 1.0, where |d| >= h
M6A_HD inline bool outside(int64_t d, int64_t h) { return d >= h || -d >= h; }

M6A_HD inline int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0)) ? 1 : 0); }   // b > 0 here

// the cells of row i inside the band are j_lo(i) <= j <= j_hi(i), clamped to the grid (an empty row has j_lo > j_hi): m i - h < n j < m i + h.
// Both do not decrease with i; h >= 1
M6A_HD inline int64_t j_lo(int64_t n, int64_t m, int64_t h, int64_t i)
{
    const int64_t j = floor_div(m * i - h, n) + 1;
    return j < 0 ? 0 : j;
}
M6A_HD inline int64_t j_hi(int64_t n, int64_t m, int64_t h, int64_t i)
{
    const int64_t j = -floor_div(-(m * i + h), n) - 1;       // ceil(...) - 1
    return j > m ? m : j;
}

// an inside cell other than (n, m): rows_left = n - i, cols_left = m - j and steps_left = n + m - i - j as doubles (exact), below =
// v[i+1][j], right = v[i][j+1].  Two products, one sum, one division
M6A_HD inline double cell(double rows_left, double below, double cols_left, double right, double steps_left)
{
    const double a = rows_left * below;
    const double b = cols_left * right;
    const double s = a + b;
    return s / steps_left;
}

}  // namespace m6a_kse

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

namespace m6a_kse {

// One item on the host; row is the caller's scratch (reused from item to item).
inline double p_value(int64_t n, int64_t m, int64_t h, std::vector<double> &row)
{
    if (undefined(n, m, h)) return not_a_number();
    if (h == 0) return 1.0;                                     // (0, 0) is outside
    if (m > n) { const int64_t t = n; n = m; m = t; }           // the shorter bag on j: the same bits
    h = clamp_h(n, m, h);
    row.assign((size_t)m + 2, 1.0);                             // row[j] = v[i][j] of the row at hand, 1.0 wherever it is outside
    row[(size_t)m + 1] = 0.0;                                   // beyond the grid
    int64_t hi_above = m;                                       // j_hi of the row before (above n: nothing to reset)
    for (int64_t i = n; i >= 0; i--) {
        const int64_t lo = j_lo(n, m, h, i), hi = j_hi(n, m, h, i);
        for (int64_t j = hi + 1; j <= hi_above; j++) row[(size_t)j] = 1.0;   // the cells the band has left; none of them is read as v[i+1][.] again
        hi_above = hi;
        const double rows_left = (double)(n - i);
        for (int64_t j = hi; j >= lo; j--) {                    // row[j] is still v[i+1][j], row[j+1] already v[i][j+1]
            const double below = i == n ? 0.0 : row[(size_t)j];
            row[(size_t)j] = i == n && j == m ? 0.0 : cell(rows_left, below, (double)(m - j), row[(size_t)j + 1], (double)(n + m - i - j));
        }
    }
    return row[0];
}

}  // namespace m6a_kse
#endif

#endif
