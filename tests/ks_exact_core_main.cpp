// The host side of m6a_ks_exact as a program of its own: m6a_ks_exact.h's p_value -- the caps, the band, the one row updated in place --
// which tests/test_ks_exact_core.py builds with ASan and UBSan and runs.  The row is the core's own heap scratch, reused from item to
// item as m6a_io_ks_exact reuses it, so a read or a write before or past it is a sanitizer report.  Every result is held, bit for bit,
// to the recurrence evaluated here over the whole (n + 1) x (m + 1) table with no band, no swap and no row reuse.  Prints one line per
// group and returns 0 when all of them hold.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "m6a_ks_exact.h"

namespace {

int g_bad = 0;

// include/m6a.h's recurrence as it is written there
double by_table(int64_t n, int64_t m, int64_t h)
{
    if (n < 1 || m < 1 || h < 0 || (n < m ? n : m) > M6A_KS_EXACT_SHORT || n * m > M6A_KS_EXACT_CELLS) return NAN;
    std::vector<double> v((size_t)((n + 1) * (m + 1)));
    auto at = [&](int64_t i, int64_t j) -> double { return i > n || j > m ? 0.0 : v[(size_t)(i * (m + 1) + j)]; };
    for (int64_t i = n; i >= 0; i--)
        for (int64_t j = m; j >= 0; j--) {
            const int64_t d = m * i - n * j;
            double x;
            if ((d < 0 ? -d : d) >= h) x = 1.0;
            else if (i == n && j == m) x = 0.0;
            else x = ((double)(n - i) * at(i + 1, j) + (double)(m - j) * at(i, j + 1)) / (double)(n + m - i - j);
            v[(size_t)(i * (m + 1) + j)] = x;
        }
    return v[0];
}

bool same_double(double x, double y)
{
    if (std::isnan(x) || std::isnan(y)) return std::isnan(x) && std::isnan(y);
    return memcmp(&x, &y, sizeof(double)) == 0;
}

void check(const char *group, int64_t n, int64_t m, int64_t h, std::vector<double> &row)
{
    const double got = m6a_kse::p_value(n, m, h, row), want = by_table(n, m, h);
    if (!same_double(got, want)) {
        g_bad++;
        printf("%s: n = %" PRId64 ", m = %" PRId64 ", h = %" PRId64 ": got %.17g, want %.17g\n", group, n, m, h, got, want);
    }
    if (!same_double(got, m6a_kse::p_value(m, n, h, row))) {
        g_bad++;
        printf("%s: n = %" PRId64 ", m = %" PRId64 ", h = %" PRId64 ": the bags swapped give other bits\n", group, n, m, h);
    }
}

}  // namespace

int main()
{
    std::vector<double> row;
    for (int64_t n = 0; n <= 14; n++)                            // every small grid and every h from the undefined -1 to past the grid
        for (int64_t m = 0; m <= 14; m++)
            for (int64_t h = -1; h <= n * m + 2; h++) check("small", n, m, h, row);
    puts("small: done");
    const int64_t edges[] = {1, 2, 20, 63, 64, 65, 127, 128, 129, 192, 193};   // the kernel's stripe of 64 rows
    for (int64_t n : edges)
        for (int64_t m : edges)
            for (int64_t h : {(int64_t)1, n * m / 7 + 1, n * m / 4, n * m / 2, n * m, n * m + 1}) check("edges", n, m, h, row);
    puts("edges: done");
    check("shrinking", 300, 280, 20000, row);                    // the scratch shrinks and grows from item to item
    check("shrinking", 2, 1, 1, row);
    check("shrinking", 1, 700, 350, row);
    check("shrinking", 2047, 3, 1500, row);
    puts("shrinking: done");
    {                                                            // the caps, and arguments no product of which may be formed
        const struct { int64_t n, m, h; bool nan; } caps[] = {
            {2047, 2047, 2047, false}, {2048, 2048, 2048, true}, {2048, 3000, 5, true}, {50000, 2000, 4000, false}, {50001, 2000, 4000, true},
            {2000, 50001, 4000, true}, {100000000, 1, 3, false}, {100000001, 1, 3, true}, {(int64_t)1 << 62, 2047, 5, true},
            {(int64_t)1 << 40, (int64_t)1 << 40, 5, true}, {20, 20, (int64_t)1 << 62, false}, {20, 20, INT64_MAX, false}, {20, 20, INT64_MIN, true},
            {0, 5, 1, true}, {5, 0, 1, true}, {-7, 5, 1, true}, {INT64_MIN, INT64_MIN, 1, true}, {INT64_MAX, INT64_MAX, INT64_MAX, true}};
        for (const auto &c : caps) {
            const double p = m6a_kse::p_value(c.n, c.m, c.h, row);
            if (std::isnan(p) != c.nan || (!c.nan && !(p >= 0.0 && p <= 1.0))) {
                g_bad++;
                printf("caps: n = %" PRId64 ", m = %" PRId64 ", h = %" PRId64 ": p = %.17g\n", c.n, c.m, c.h, p);
            }
        }
        if (m6a_kse::p_value(20, 20, (int64_t)1 << 62, row) != 0.0 || m6a_kse::p_value(20, 20, 0, row) != 1.0) { g_bad++; puts("caps: h beyond the grid is not 0.0, or h = 0 not 1.0"); }
        const double sub = m6a_kse::p_value(520, 520, 520 * 520, row), zero = m6a_kse::p_value(600, 600, 600 * 600, row);
        if (!(sub > 0.0 && sub < 2.2250738585072014e-308) || zero != 0.0) { g_bad++; printf("caps: subnormal %.17g, zero %.17g\n", sub, zero); }
    }
    puts("caps: done");
    printf("%d failures\n", g_bad);
    return g_bad ? 1 : 0;
}
