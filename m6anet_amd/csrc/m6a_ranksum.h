// m6a_ranksum.h -- the per-site rank-sum test between two conditions (include/m6a.h: m6a_site_ranksum), the part both sides share.
// Plain C++ marked for host and device: m6a_ranksum.hip compiles finish() and undefined() for gfx950 behind its counting kernel,
// m6a_io.cpp compiles all of it for the CPU (m6a_io_site_ranksum), and tests/ranksum_core_main.cpp runs it as a program of its own
// under ASan and UBSan.  The three counts are integers, so any way of counting gives the same bits; z is the one order of IEEE double
// operations the header states, each evaluated as written (the builds pass -ffp-contract=off; division and sqrt round correctly).
//   count()   one pair on the host: both bags sorted into copies, then one merge walk over the distinct values -- exact, O(N log N),
//             so the largest defined pair (n + m = 2^20) is as cheap to check as a small one.
#ifndef M6A_RANKSUM_H
#define M6A_RANKSUM_H
#include <stdint.h>
#include <math.h>

#ifndef M6A_HD
#if defined(__HIPCC__)
#define M6A_HD __host__ __device__
#else
#define M6A_HD
#endif
#endif

namespace m6a_ranksum {

constexpr int64_t kMaxPooled = (int64_t)1 << 20;          // n + m above this: the pair is undefined (tie <= N^3 stays inside int64)

struct Result { int64_t gt, eq, tie; double z; };

// either bag empty or the pooled sample too large (a NaN in a bag is the third reason: the counting finds it)
M6A_HD inline bool undefined_sizes(int64_t n, int64_t m) { return n <= 0 || m <= 0 || n + m > kMaxPooled; }

M6A_HD inline Result undefined()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return {-1, -1, -1, __builtin_nan("")};
#else
    return {-1, -1, -1, NAN};
#endif
}

// z of a defined pair from its counts (include/m6a.h states these lines)
M6A_HD inline double finish(int64_t n, int64_t m, int64_t gt, int64_t eq, int64_t tie)
{
    const double nm = (double)n * (double)m;
    const double N = (double)(n + m);
    const double U = (double)(2 * gt + eq) * 0.5;
    const double d = U - nm * 0.5;
    const double tc = (double)tie / (N * (N - 1.0));
    const double var = nm / 12.0 * ((N + 1.0) - tc);
#if defined(__HIP_DEVICE_COMPILE__)
    const double s = __dsqrt_rn(var);
#else
    const double s = sqrt(var);
#endif
    const double a = fabs(d) - 0.5;
    const double num = a > 0.0 ? a : 0.0;
    return num > 0.0 ? copysign(num, d) / s : copysign(0.0, d);
}

}  // namespace m6a_ranksum

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>

namespace m6a_ranksum {

// One pair on the host.  a [n] and b [m] are read, never written; sa and sb are the caller's scratch (reused from pair to pair).
inline Result count(const float *a, int64_t n, const float *b, int64_t m, std::vector<float> &sa, std::vector<float> &sb)
{
    if (undefined_sizes(n, m)) return undefined();
    for (int64_t i = 0; i < n; i++) if (a[i] != a[i]) return undefined();
    for (int64_t j = 0; j < m; j++) if (b[j] != b[j]) return undefined();
    sa.assign(a, a + n);
    sb.assign(b, b + m);
    std::sort(sa.begin(), sa.end());                          // float <: -0.0 and 0.0 are one value, as == has them
    std::sort(sb.begin(), sb.end());
    int64_t gt = 0, eq = 0, tie = 0, i = 0, j = 0;
    while (i < n || j < m) {
        const float v = (j >= m || (i < n && sa[(size_t)i] <= sb[(size_t)j])) ? sa[(size_t)i] : sb[(size_t)j];   // the smallest value left
        int64_t ca = 0, cb = 0;
        while (i + ca < n && sa[(size_t)(i + ca)] == v) ca++;
        while (j + cb < m && sb[(size_t)(j + cb)] == v) cb++;
        gt += ca * j;                                         // every b before j is below v
        eq += ca * cb;
        const int64_t t = ca + cb;
        tie += t * t * t - t;
        i += ca;
        j += cb;
    }
    return {gt, eq, tie, finish(n, m, gt, eq, tie)};
}

// Column c of the rows X [n][width], gathered into the caller's scratch g (m6a_ks.h gathers with it too).  Reads X[i * width + c] and
// nothing else.
inline const float *gather_column(const float *X, int64_t n, int c, int width, std::vector<float> &g)
{
    g.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) g[(size_t)i] = X[i * width + c];
    return g.data();
}

// One pair and one column of m6a_site_signal_ranksum on the host: column c of the rows Xa [n][width] and Xb [m][width], gathered into
// the caller's scratch ga and gb and counted as above.
inline Result count_column(const float *Xa, int64_t n, const float *Xb, int64_t m, int c, int width, std::vector<float> &ga,
                           std::vector<float> &gb, std::vector<float> &sa, std::vector<float> &sb)
{
    if (undefined_sizes(n, m)) return undefined();
    return count(gather_column(Xa, n, c, width, ga), n, gather_column(Xb, m, c, width, gb), m, sa, sb);
}

}  // namespace m6a_ranksum
#endif

#endif
