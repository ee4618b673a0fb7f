// norm_core_main.cpp -- m6anet_amd/csrc/m6a_norm.h as a program of its own, for the sanitizers (tests/test_norm_factors.py builds it
// with -fsanitize=address,undefined and runs it as a child process).
//
// The first file holds doubles, 8 bytes each; the second int64 lengths.  For every length n, a heap allocation of exactly n doubles
// is filled with the file's first n values at a stride of nine (a column of [n][9] rows, as the loader and the kernels read it), so an
// element read past the column is a sanitizer report.  One line per length, the bits in hexadecimal:
//   <n>\t<colsum of the values>\t<colsum of the squares>\t<mean>\t<std>      mean and std: finish(both sums, n)
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "m6a_norm.h"

namespace {

template <class T> bool read_file(const char *path, std::vector<T> &d)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    T buf[4096];
    size_t got;
    d.clear();
    while ((got = fread(buf, sizeof(T), 4096, f)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(f);
    return true;
}

uint64_t bits(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}

}  // namespace

int main(int argc, char **argv)
{
    std::vector<double> v;
    std::vector<int64_t> lens;
    if (argc != 3 || !read_file(argv[1], v) || !read_file(argv[2], lens)) {
        fprintf(stderr, "usage: norm_core <doubles> <int64 lengths>\n");
        return 2;
    }
    for (int64_t n : lens) {
        if (n < 0 || (size_t)n > v.size()) return 1;
        // the column is element 4 of rows of nine; the allocation ends with the column's last element
        const size_t cells = n ? (size_t)(9 * (n - 1) + 5) : 1;
        std::unique_ptr<double[]> rows(new double[cells]());
        for (int64_t r = 0; r < n; r++) rows[(size_t)(9 * r + 4)] = v[(size_t)r];
        const double *col = rows.get() + 4;
        const double s = m6a_norm::colsum([&](int64_t r) { return col[9 * r]; }, n);
        const double s2 = m6a_norm::colsum([&](int64_t r) { const double x = col[9 * r]; return x * x; }, n);
        double mean = 0, sd = 0;
        if (n) m6a_norm::finish(s, s2, n, &mean, &sd);
        printf("%" PRId64 "\t%016" PRIx64 "\t%016" PRIx64 "\t%016" PRIx64 "\t%016" PRIx64 "\n", n, bits(s), bits(s2), bits(mean), bits(sd));
    }
    return 0;
}
