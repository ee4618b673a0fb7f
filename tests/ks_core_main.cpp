// The host side of m6a_site_ks and m6a_site_signal_ks as a program of its own: m6a_ks.h's count and count_column -- the sorted copies,
// the merge walk, the two middles, the gather of one column of rows [n][9] -- which tests/test_ks_core.py builds with ASan and UBSan and
// runs.  Every bag is copied into a heap allocation of exactly its size first, so a read before or past it is a sanitizer report, and
// every result is held to the definition counted here over all pairs of values and to a median found by counting, not by sorting.  Bags
// of 0 to 300 reads, with and without NaN, signed zeros and infinities.  Prints one line per group and returns 0 when all of them hold.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "m6a_ks.h"

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

// the k-th order statistic by counting: the value x with #{< x} <= k < #{<= x}
float order_statistic(const std::vector<float> &v, int64_t k)
{
    for (float x : v) {
        int64_t lt = 0, le = 0;
        for (float y : v) { lt += y < x; le += y <= x; }
        if (lt <= k && k < le) return x;
    }
    return NAN;
}

double median_by_counting(const std::vector<float> &v)
{
    const int64_t s = (int64_t)v.size();
    const double med = (double)order_statistic(v, (s - 1) / 2) * 0.5 + (double)order_statistic(v, s / 2) * 0.5;
    return med == 0.0 ? 0.0 : med;
}

m6a_ks::Result by_definition(const std::vector<float> &a, const std::vector<float> &b)
{
    const int64_t n = (int64_t)a.size(), m = (int64_t)b.size();
    if (m6a_ranksum::undefined_sizes(n, m)) return m6a_ks::undefined();
    for (float x : a) if (x != x) return m6a_ks::undefined();
    for (float x : b) if (x != x) return m6a_ks::undefined();
    std::vector<float> pooled(a);
    pooled.insert(pooled.end(), b.begin(), b.end());
    int64_t d_pos = INT64_MIN, d_neg = INT64_MIN;
    for (float v : pooled) {
        int64_t A = 0, B = 0;
        for (float x : a) A += x <= v;
        for (float y : b) B += y <= v;
        const int64_t t = m * A - n * B;
        if (t > d_pos) d_pos = t;
        if (-t > d_neg) d_neg = -t;
    }
    return {d_pos, d_neg, median_by_counting(a), median_by_counting(b)};
}

bool same_double(double x, double y)
{
    if (std::isnan(x) || std::isnan(y)) return std::isnan(x) && std::isnan(y);
    return memcmp(&x, &y, sizeof(double)) == 0;
}

bool same(const m6a_ks::Result &x, const m6a_ks::Result &y)
{
    return x.d_pos == y.d_pos && x.d_neg == y.d_neg && same_double(x.med_a, y.med_a) && same_double(x.med_b, y.med_b);
}

void report(const char *group, size_t n, size_t m, int c, const m6a_ks::Result &got, const m6a_ks::Result &want)
{
    g_bad++;
    printf("%s: n = %zu, m = %zu, column %d: got %" PRId64 " %" PRId64 " %.17g %.17g, want %" PRId64 " %" PRId64 " %.17g %.17g\n", group, n, m, c,
           got.d_pos, got.d_neg, got.med_a, got.med_b, want.d_pos, want.d_neg, want.med_a, want.med_b);
}

// one pair of bags of values; returns whether it is undefined
bool check(const char *group, const std::vector<float> &a, const std::vector<float> &b, std::vector<float> &sa, std::vector<float> &sb)
{
    const std::unique_ptr<float[]> pa = exact(a), pb = exact(b);
    const m6a_ks::Result got = m6a_ks::count(pa.get(), (int64_t)a.size(), pb.get(), (int64_t)b.size(), sa, sb);
    const m6a_ks::Result want = by_definition(a, b);
    if (!same(got, want)) report(group, a.size(), b.size(), -1, got, want);
    if (got.d_pos >= 0 && (got.d_neg < 0 || (got.med_a == 0.0 && std::signbit(got.med_a)) || (got.med_b == 0.0 && std::signbit(got.med_b)))) {
        g_bad++;
        printf("%s: a negative d_neg or a negative zero median\n", group);
    }
    return got.d_pos < 0;
}

// every column of one pair of bags of rows, the scratch reused from column to column as m6a_io_site_signal_ks reuses it; returns the
// columns undefined
int check_rows(const char *group, const std::vector<float> &A, const std::vector<float> &B, std::vector<float> &ga, std::vector<float> &gb,
               std::vector<float> &sa, std::vector<float> &sb)
{
    const std::unique_ptr<float[]> pa = exact(A), pb = exact(B);
    const int64_t n = (int64_t)A.size() / C, m = (int64_t)B.size() / C;
    int undefined = 0;
    for (int c = 0; c < C; c++) {
        const m6a_ks::Result got = m6a_ks::count_column(pa.get(), n, pb.get(), m, c, C, ga, gb, sa, sb);
        std::vector<float> a, b;
        for (int64_t i = 0; i < n; i++) a.push_back(A[(size_t)(i * C + c)]);
        for (int64_t j = 0; j < m; j++) b.push_back(B[(size_t)(j * C + c)]);
        const m6a_ks::Result want = by_definition(a, b);
        undefined += got.d_pos < 0;
        if (!same(got, want)) report(group, (size_t)n, (size_t)m, c, got, want);
    }
    return undefined;
}

const float few[] = {0.0f, 0.25f, 0.5f, 1.0f, -0.0f, INFINITY, -INFINITY};

// family 0: four values; 1: those with signed zeros and infinities; 2: 24 random bits
float draw_one(int family)
{
    return family == 0 ? few[next_u32() % 4] : family == 1 ? few[next_u32() % 7] : (float)(next_u32() >> 8) * (1.0f / 16777216.0f);
}

std::vector<float> draw(size_t n, int family)
{
    std::vector<float> v(n);
    for (float &x : v) x = draw_one(family);
    return v;
}

std::vector<float> draw_rows(size_t n)
{
    std::vector<float> v(n * C);
    for (size_t i = 0; i < n; i++)
        for (int c = 0; c < C; c++) v[i * C + c] = draw_one(c % 3);
    return v;
}

}  // namespace

int main()
{
    std::vector<float> ga, gb, sa, sb;
    for (size_t n = 0; n <= 6; n++)                          // every small size, empty bags included, odd and even
        for (size_t m = 0; m <= 6; m++)
            for (int rep = 0; rep < 12; rep++) {
                const bool undefined = check("small", draw(n, rep % 3), draw(m, (rep / 3) % 3), sa, sb);
                if (undefined != (n == 0 || m == 0)) { g_bad++; printf("small: undefined = %d at n = %zu, m = %zu\n", (int)undefined, n, m); }
                const int columns = check_rows("small rows", draw_rows(n), draw_rows(m), ga, gb, sa, sb);
                if (columns != (n == 0 || m == 0 ? C : 0)) { g_bad++; printf("small rows: %d columns undefined at n = %zu, m = %zu\n", columns, n, m); }
            }
    puts("small: done");
    const size_t edges[] = {1, 19, 20, 21, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300};   // the kernel's chunk of 64 and tile of 256
    for (size_t n : edges)
        for (size_t m : edges) {
            check("edges", draw(n, (int)(n % 3)), draw(m, (int)(m % 3)), sa, sb);
            if (n <= 65 || m <= 65) check_rows("edges rows", draw_rows(n), draw_rows(m), ga, gb, sa, sb);
        }
    check_rows("shrinking", draw_rows(300), draw_rows(300), ga, gb, sa, sb);                   // the scratch shrinks from pair to pair
    check_rows("shrinking", draw_rows(2), draw_rows(0), ga, gb, sa, sb);
    check_rows("shrinking", draw_rows(3), draw_rows(1), ga, gb, sa, sb);
    puts("edges: done");
    {                                                        // the middles the statement names
        const m6a_ks::Result zero = m6a_ks::count(exact({1.0f, 0.0f, -1.0f, -0.0f}).get(), 4, exact({-0.0f, -0.0f, -0.0f}).get(), 3, sa, sb);
        if (zero.med_a != 0.0 || std::signbit(zero.med_a) || zero.med_b != 0.0 || std::signbit(zero.med_b)) { g_bad++; puts("middles: a zero median is not +0.0"); }
        const m6a_ks::Result inf = m6a_ks::count(exact({INFINITY, -INFINITY, -INFINITY, INFINITY}).get(), 4, exact({0.5f, INFINITY, -INFINITY}).get(), 3, sa, sb);
        if (inf.d_pos < 0 || !std::isnan(inf.med_a) || inf.med_b != 0.5) { g_bad++; puts("middles: -inf and +inf do not give NaN in a defined pair"); }
        check("middles", {1.0f, 0.0f, -1.0f, -0.0f}, {-0.0f, -0.0f, -0.0f}, sa, sb);
        check("middles", {INFINITY, -INFINITY, -INFINITY, INFINITY}, {0.5f, INFINITY, -INFINITY}, sa, sb);
    }
    puts("middles: done");
    for (int side = 0; side < 2; side++)                     // a NaN in either bag, first and last read: undefined
        for (size_t n : {(size_t)1, (size_t)5, (size_t)300})
            for (size_t at : {(size_t)0, n - 1}) {
                std::vector<float> x = draw(n, 2), y = draw(7, 2);
                x[at] = NAN;
                if (!(side ? check("nan in b", y, x, sa, sb) : check("nan in a", x, y, sa, sb))) { g_bad++; puts("nan: a pair with a NaN is defined"); }
            }
    for (int c = 0; c < C; c++)                              // a NaN in column c of either bag of rows: that column alone
        for (int side = 0; side < 2; side++)
            for (size_t n : {(size_t)1, (size_t)5, (size_t)70}) {
                std::vector<float> A = draw_rows(n), B = draw_rows(7);
                for (size_t row : {(size_t)0, n - 1}) {
                    std::vector<float> X = A;
                    X[row * C + (size_t)c] = NAN;
                    const int undefined = side ? check_rows("nan in b", B, X, ga, gb, sa, sb) : check_rows("nan in a", X, B, ga, gb, sa, sb);
                    if (undefined != 1) { g_bad++; printf("nan: %d columns undefined for a NaN in column %d\n", undefined, c); }
                }
            }
    puts("nan: done");
    printf("%d failures\n", g_bad);
    return g_bad ? 1 : 0;
}
