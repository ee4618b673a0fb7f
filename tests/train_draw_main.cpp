// The read draw of the training step (m6anet_amd/csrc/m6a_train_draw.h) as a program of its own: tests/test_train_draw_core.py builds it
// with ASan and UBSan and holds its output to tests/train_statement.py.
//   draws FILE               every line of FILE is "seed i n bag": prints the bag site-local read numbers, space separated
//   hist seed n bag count    positions i = 0 .. count - 1: prints bag lines, line j = how often draw j gave each of the n read numbers
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "m6a_train_draw.h"

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "draws")) {
        FILE *f = fopen(argv[2], "r");
        if (!f) return 2;
        uint64_t seed, i, n;
        int bag;
        while (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %d", &seed, &i, &n, &bag) == 4) {
            if (bag < 1 || bag > m6a_train_draw::kMaxBag || n < (uint64_t)bag || n > 0xffffffffull) { fclose(f); return 3; }
            std::vector<int64_t> out((size_t)bag);              // exactly bag entries: a write past them is caught
            m6a_train_draw::draw(seed, i, n, bag, out.data());
            for (int j = 0; j < bag; j++) printf(j ? " %" PRId64 : "%" PRId64, out[(size_t)j]);
            printf("\n");
        }
        fclose(f);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "hist")) {
        const uint64_t seed = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10), count = strtoull(argv[5], nullptr, 10);
        const int bag = atoi(argv[4]);
        if (bag < 1 || bag > m6a_train_draw::kMaxBag || n < (uint64_t)bag || n > 100000) return 3;
        std::vector<int64_t> hist((size_t)bag * n, 0), out((size_t)bag);
        for (uint64_t i = 0; i < count; i++) {
            m6a_train_draw::draw(seed, i, n, bag, out.data());
            for (int j = 0; j < bag; j++) hist[(size_t)j * n + (size_t)out[(size_t)j]]++;
        }
        for (int j = 0; j < bag; j++) {
            for (uint64_t v = 0; v < n; v++) printf(v ? " %" PRId64 : "%" PRId64, hist[(size_t)j * n + v]);
            printf("\n");
        }
        return 0;
    }
    return 1;
}
