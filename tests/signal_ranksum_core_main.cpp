// The host side of m6a_site_signal_ranksum as a program of its own: m6a_ranksum.h's count_column -- the gather of one column of two
// bags of rows [n][9] and the count behind it -- which tests/test_signal_ranksum_core.py builds with ASan and UBSan and runs.  Every
// bag is copied into a heap allocation of exactly its size first, so a read before or past its rows is a sanitizer report, and every
// result is held to the definition counted here over all pairs of the column's values.  Bags of 0 to 300 rows, with and without NaN
// columns.  Prints one line per group and returns 0 when all of them hold.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "m6a_ranksum.h"

namespace {

constexpr int C = 9;
int g_bad = 0;

// xorshift: the program needs no library generator
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t next_u32()
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}

std::unique_ptr<float[]> exact(const std::vector<float> &v)
{
    std::unique_ptr<float[]> p(new float[v.size()]);        // size 0: a valid pointer to nothing
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(float));
    return p;
}

m6a_ranksum::Result by_definition(const std::vector<float> &A, const std::vector<float> &B, int c)
{
    const int64_t n = (int64_t)A.size() / C, m = (int64_t)B.size() / C;
    if (m6a_ranksum::undefined_sizes(n, m)) return m6a_ranksum::undefined();
    std::vector<float> a, b;
    for (int64_t i = 0; i < n; i++) a.push_back(A[(size_t)(i * C + c)]);
    for (int64_t j = 0; j < m; j++) b.push_back(B[(size_t)(j * C + c)]);
    for (float x : a) if (x != x) return m6a_ranksum::undefined();
    for (float x : b) if (x != x) return m6a_ranksum::undefined();
    int64_t gt = 0, eq = 0, tie = 0;
    for (float x : a) for (float y : b) { gt += x > y; eq += x == y; }
    std::vector<float> pooled(a);
    pooled.insert(pooled.end(), b.begin(), b.end());
    for (float x : pooled) {
        int64_t t = 0;
        for (float y : pooled) t += x == y;
        tie += t * t - 1;
    }
    return {gt, eq, tie, m6a_ranksum::finish(n, m, gt, eq, tie)};
}

bool same(const m6a_ranksum::Result &x, const m6a_ranksum::Result &y)
{
    if (x.gt != y.gt || x.eq != y.eq || x.tie != y.tie) return false;
    if (std::isnan(x.z) || std::isnan(y.z)) return std::isnan(x.z) && std::isnan(y.z);
    return memcmp(&x.z, &y.z, sizeof(double)) == 0;
}

// every column of one pair, the scratch reused from column to column as m6a_io_site_signal_ranksum reuses it; returns the columns undefined
int check(const char *group, const std::vector<float> &A, const std::vector<float> &B, std::vector<float> &ga, std::vector<float> &gb,
          std::vector<float> &sa, std::vector<float> &sb)
{
    const std::unique_ptr<float[]> pa = exact(A), pb = exact(B);
    int undefined = 0;
    for (int c = 0; c < C; c++) {
        const m6a_ranksum::Result got = m6a_ranksum::count_column(pa.get(), (int64_t)A.size() / C, pb.get(), (int64_t)B.size() / C, c, C, ga, gb, sa, sb);
        const m6a_ranksum::Result want = by_definition(A, B, c);
        undefined += got.gt < 0;
        if (!same(got, want)) {
            g_bad++;
            printf("%s: n = %zu, m = %zu, column %d: got %" PRId64 " %" PRId64 " %" PRId64 " %.17g, want %" PRId64 " %" PRId64 " %" PRId64 " %.17g\n",
                   group, A.size() / C, B.size() / C, c, got.gt, got.eq, got.tie, got.z, want.gt, want.eq, want.tie, want.z);
        }
    }
    return undefined;
}

// n rows: column c draws from a family of its own -- few values, few values with signed zeros and infinities, or 24 random bits
std::vector<float> draw(size_t n)
{
    static const float few[] = {0.0f, 0.25f, 0.5f, 1.0f, -0.0f, INFINITY, -INFINITY};
    std::vector<float> v(n * C);
    for (size_t i = 0; i < n; i++)
        for (int c = 0; c < C; c++)
            v[i * C + c] = c % 3 == 0 ? few[next_u32() % 4] : c % 3 == 1 ? few[next_u32() % 7] : (float)(next_u32() >> 8) * (1.0f / 16777216.0f);
    return v;
}

}  // namespace

int main()
{
    std::vector<float> ga, gb, sa, sb;
    for (size_t n = 0; n <= 5; n++)                          // every small size, empty bags included
        for (size_t m = 0; m <= 5; m++)
            for (int rep = 0; rep < 8; rep++) {
                const int undefined = check("small", draw(n), draw(m), ga, gb, sa, sb);
                if (undefined != (n == 0 || m == 0 ? C : 0)) { g_bad++; printf("small: %d columns undefined at n = %zu, m = %zu\n", undefined, n, m); }
            }
    puts("small: done");
    const size_t edges[] = {1, 19, 20, 21, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300};   // the kernel's chunk of 64 and tile of 256
    for (size_t n : edges)
        for (size_t m : edges) check("edges", draw(n), draw(m), ga, gb, sa, sb);
    check("shrinking", draw(300), draw(300), ga, gb, sa, sb);                                  // the scratch shrinks from pair to pair
    check("shrinking", draw(2), draw(0), ga, gb, sa, sb);
    check("shrinking", draw(3), draw(1), ga, gb, sa, sb);
    puts("edges: done");
    for (int c = 0; c < C; c++)                              // a NaN in column c of either bag, first and last row: that column alone
        for (int side = 0; side < 2; side++)
            for (size_t n : {(size_t)1, (size_t)5, (size_t)300}) {
                std::vector<float> A = draw(n), B = draw(7);
                for (size_t row : {(size_t)0, n - 1}) {
                    std::vector<float> X = A;
                    X[row * C + (size_t)c] = NAN;
                    const int undefined = side ? check("nan in b", B, X, ga, gb, sa, sb) : check("nan in a", X, B, ga, gb, sa, sb);
                    if (undefined != 1) { g_bad++; printf("nan: %d columns undefined for a NaN in column %d\n", undefined, c); }
                }
            }
    {
        std::vector<float> A = draw(40), B = draw(33);
        for (int c = 0; c < C; c++) (c % 2 ? A : B)[(size_t)((7 * c) % 33 * C + c)] = NAN;
        if (check("nan in every column", A, B, ga, gb, sa, sb) != C) { g_bad++; puts("nan in every column: a column is defined"); }
    }
    puts("nan: done");
    printf("%d failures\n", g_bad);
    return g_bad ? 1 : 0;
}
