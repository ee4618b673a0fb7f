// The rank-sum core (m6anet_amd/csrc/m6a_ranksum.h) as a program of its own: tests/test_ranksum_core.py builds it with ASan and UBSan
// and runs it.  Every bag is copied into a heap allocation of exactly its size first, so a read before or past a bag is a sanitizer
// report, and every result is held to the definition counted here over all pairs (or, at the 2^20 bound, to the closed form of a
// sample of one or two values).  Prints one line per group and returns 0 when all of them hold.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "m6a_ranksum.h"

namespace {

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

m6a_ranksum::Result by_definition(const std::vector<float> &a, const std::vector<float> &b)
{
    const int64_t n = (int64_t)a.size(), m = (int64_t)b.size();
    if (m6a_ranksum::undefined_sizes(n, m)) return m6a_ranksum::undefined();
    for (float x : a) if (x != x) return m6a_ranksum::undefined();
    for (float x : b) if (x != x) return m6a_ranksum::undefined();
    int64_t gt = 0, eq = 0, tie = 0;
    for (float x : a) for (float y : b) { gt += x > y; eq += x == y; }
    std::vector<float> pooled(a);
    pooled.insert(pooled.end(), b.begin(), b.end());
    for (float x : pooled) {
        int64_t c = 0;
        for (float y : pooled) c += x == y;
        tie += c * c - 1;
    }
    return {gt, eq, tie, m6a_ranksum::finish(n, m, gt, eq, tie)};
}

bool same(const m6a_ranksum::Result &x, const m6a_ranksum::Result &y)
{
    if (x.gt != y.gt || x.eq != y.eq || x.tie != y.tie) return false;
    if (std::isnan(x.z) || std::isnan(y.z)) return std::isnan(x.z) && std::isnan(y.z);
    return memcmp(&x.z, &y.z, sizeof(double)) == 0;
}

m6a_ranksum::Result run(const std::vector<float> &a, const std::vector<float> &b)
{
    const std::unique_ptr<float[]> pa = exact(a), pb = exact(b);
    std::vector<float> sa, sb;
    return m6a_ranksum::count(pa.get(), (int64_t)a.size(), pb.get(), (int64_t)b.size(), sa, sb);
}

void check(const char *group, const std::vector<float> &a, const std::vector<float> &b)
{
    const m6a_ranksum::Result got = run(a, b), want = by_definition(a, b);
    if (!same(got, want)) {
        g_bad++;
        printf("%s: n = %zu, m = %zu: got %" PRId64 " %" PRId64 " %" PRId64 " %.17g, want %" PRId64 " %" PRId64 " %" PRId64 " %.17g\n", group,
               a.size(), b.size(), got.gt, got.eq, got.tie, got.z, want.gt, want.eq, want.tie, want.z);
    }
}

std::vector<float> draw(size_t n, int kind)
{
    static const float few[] = {0.0f, 0.25f, 0.5f, 1.0f, -0.0f, INFINITY, -INFINITY};
    std::vector<float> v(n);
    for (float &x : v) x = kind == 0 ? few[next_u32() % 4] : kind == 1 ? few[next_u32() % 7] : (float)(next_u32() >> 8) * (1.0f / 16777216.0f);
    return v;
}

}  // namespace

int main()
{
    for (size_t n = 0; n <= 5; n++)                          // every small size, empty bags included, on every kind of value
        for (size_t m = 0; m <= 5; m++)
            for (int kind = 0; kind < 3; kind++)
                for (int rep = 0; rep < 8; rep++) check("small", draw(n, kind), draw(m, kind));
    puts("small: done");
    const size_t edges[] = {1, 19, 20, 21, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513};   // the kernel's chunk of 64 and tile of 256
    for (size_t n : edges)
        for (size_t m : edges) check("edges", draw(n, (int)((n + m) % 3)), draw(m, (int)((n + 2 * m) % 3)));
    puts("edges: done");
    check("all equal", std::vector<float>(70, 0.5f), std::vector<float>(33, 0.5f));
    check("signed zeros", {-0.0f, 0.0f, -0.0f, 0.25f}, {0.0f, -0.0f, 0.5f});
    for (size_t at = 0; at < 5; at++) {                      // a NaN at every place of either bag
        std::vector<float> a = draw(5, 2), b = draw(5, 2);
        a[at] = NAN;
        check("nan in a", a, b);
        check("nan in b", b, a);
    }
    puts("values: done");
    {                                                        // the bound: n + m = 2^20 is defined, one read more is not
        const int64_t h = m6a_ranksum::kMaxPooled / 2, N = 2 * h;
        const m6a_ranksum::Result one = run(std::vector<float>((size_t)h, 0.25f), std::vector<float>((size_t)h, 0.25f));
        const m6a_ranksum::Result two = run(std::vector<float>((size_t)h, 0.75f), std::vector<float>((size_t)h, 0.25f));
        const m6a_ranksum::Result over = run(std::vector<float>((size_t)h + 1, 0.75f), std::vector<float>((size_t)h, 0.25f));
        const int64_t t2 = 2 * (h * h * h - h);
        if (!same(one, {0, h * h, N * N * N - N, 0.0})) { g_bad++; puts("bound: one value"); }
        if (!same(two, {h * h, 0, t2, m6a_ranksum::finish(h, h, h * h, 0, t2)}) || !(two.z > 0)) { g_bad++; puts("bound: two values"); }
        if (!same(over, m6a_ranksum::undefined())) { g_bad++; puts("bound: 2^20 + 1 reads must be undefined"); }
    }
    puts("bound: done");
    printf("%d failures\n", g_bad);
    return g_bad ? 1 : 0;
}
