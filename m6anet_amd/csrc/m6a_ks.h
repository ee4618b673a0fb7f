// m6a_ks.h -- the per-site two-sample Kolmogorov-Smirnov integers and the two medians (include/m6a.h: m6a_site_ks), the part both
// sides share.  Plain C++ marked for host and device, as m6a_ranksum.h is: m6a_ks.hip compiles median() and undefined() for gfx950
// behind its counting kernels, m6a_io.cpp compiles all of it for the CPU (m6a_io_site_ks, m6a_io_site_signal_ks), and
// tests/ks_core_main.cpp runs it as a program of its own under ASan and UBSan.  d_pos and d_neg are integers, so any way of counting
// gives the same bits; a median is two float32 order statistics and one line of IEEE double operations, evaluated as written.
//   count()   one pair on the host: both bags sorted into copies, then one merge walk over the distinct values -- exact, O(N log N).
// What is undefined is m6a_ranksum.h's rule (undefined_sizes, a NaN), used as it is.
#ifndef M6A_KS_H
#define M6A_KS_H
#include "m6a_ranksum.h"

namespace m6a_ks {

struct Result { int64_t d_pos, d_neg; double med_a, med_b; };

M6A_HD inline Result undefined()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return {-1, -1, __builtin_nan(""), __builtin_nan("")};
#else
    return {-1, -1, NAN, NAN};
#endif
}

// the median of a bag from its two middle order statistics lo = x_((s-1)/2) and hi = x_(s/2) (include/m6a.h states this line): a result
// that compares equal to zero is +0.0, since which of -0.0 and 0.0 a selection meets is not defined; +inf and -inf give NaN
M6A_HD inline double median(float lo, float hi)
{
    const double med = (double)lo * 0.5 + (double)hi * 0.5;
    return med == 0.0 ? 0.0 : med;
}

}  // namespace m6a_ks

#if !defined(__HIP_DEVICE_COMPILE__)

namespace m6a_ks {

// One pair on the host.  a [n] and b [m] are read, never written; sa and sb are the caller's scratch (reused from pair to pair).
inline Result count(const float *a, int64_t n, const float *b, int64_t m, std::vector<float> &sa, std::vector<float> &sb)
{
    if (m6a_ranksum::undefined_sizes(n, m)) return undefined();
    for (int64_t i = 0; i < n; i++) if (a[i] != a[i]) return undefined();
    for (int64_t j = 0; j < m; j++) if (b[j] != b[j]) return undefined();
    sa.assign(a, a + n);
    sb.assign(b, b + m);
    std::sort(sa.begin(), sa.end());                          // float <: -0.0 and 0.0 are one value, as <= has them
    std::sort(sb.begin(), sb.end());
    int64_t d_pos = 0, d_neg = 0, i = 0, j = 0;
    while (i < n || j < m) {
        const float v = (j >= m || (i < n && sa[(size_t)i] <= sb[(size_t)j])) ? sa[(size_t)i] : sb[(size_t)j];   // the smallest value left
        while (i < n && sa[(size_t)i] == v) i++;              // i = A(v), j = B(v) behind the two loops
        while (j < m && sb[(size_t)j] == v) j++;
        const int64_t t = m * i - n * j;
        d_pos = std::max(d_pos, t);
        d_neg = std::max(d_neg, -t);
    }
    return {d_pos, d_neg, median(sa[(size_t)((n - 1) / 2)], sa[(size_t)(n / 2)]), median(sb[(size_t)((m - 1) / 2)], sb[(size_t)(m / 2)])};
}

// One pair and one column of m6a_site_signal_ks on the host: column c of the rows Xa [n][width] and Xb [m][width], gathered into the
// caller's scratch ga and gb (m6a_ranksum::gather_column) and counted as above.
inline Result count_column(const float *Xa, int64_t n, const float *Xb, int64_t m, int c, int width, std::vector<float> &ga,
                           std::vector<float> &gb, std::vector<float> &sa, std::vector<float> &sb)
{
    if (m6a_ranksum::undefined_sizes(n, m)) return undefined();
    return count(m6a_ranksum::gather_column(Xa, n, c, width, ga), n, m6a_ranksum::gather_column(Xb, m, c, width, gb), m, sa, sb);
}

}  // namespace m6a_ks
#endif

#endif
