// npy_core_main.cpp -- m6anet_amd/csrc/m6a_npy.h as a program of its own, for the sanitizers (tests/test_repr_file_host.py builds it
// with -fsanitize=address,undefined and runs it as a child process).
//
//   npy_core header <n_rows>...                one line per n_rows and dtype (0, then 1): <n_rows>\t<dtype>\t<the header's bytes in hex>
//   npy_core rounds <off file> <round_bytes>   the file holds off[0..S] as int64; per dtype one line: <dtype>\t<widest rows>\t<cut[0]> <cut[1]> ...
//                                              off[] is copied into a heap block of exactly S + 1 entries: a read past it is a report
//   npy_core offset <n_rows> <row>             per dtype one line: <dtype>\t<byte where the row begins>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "m6a_npy.h"

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "header")) {
        for (int i = 2; i < argc; i++)
            for (int dtype = 0; dtype < 2; dtype++) {
                const std::string h = m6a_npy::header(atoll(argv[i]), dtype);
                printf("%lld\t%d\t", atoll(argv[i]), dtype);
                for (unsigned char c : h) printf("%02x", c);
                putchar('\n');
            }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "rounds")) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) return 2;
        std::vector<int64_t> v;
        int64_t x;
        while (fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
        fclose(f);
        if (v.empty()) return 2;
        std::unique_ptr<int64_t[]> off(new int64_t[v.size()]);
        memcpy(off.get(), v.data(), v.size() * sizeof(int64_t));
        for (int dtype = 0; dtype < 2; dtype++) {
            std::vector<int64_t> cut;
            const int64_t widest = m6a_npy::cut_rounds(off.get(), (int64_t)v.size() - 1, atoll(argv[3]), dtype, cut);
            printf("%d\t%lld\t", dtype, (long long)widest);
            for (size_t i = 0; i < cut.size(); i++) printf("%s%lld", i ? " " : "", (long long)cut[i]);
            putchar('\n');
        }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "offset")) {
        for (int dtype = 0; dtype < 2; dtype++) printf("%d\t%lld\n", dtype, (long long)m6a_npy::row_offset(atoll(argv[2]), dtype, atoll(argv[3])));
        return 0;
    }
    fprintf(stderr, "usage: npy_core header <n_rows>... | rounds <off file> <round_bytes> | offset <n_rows> <row>\n");
    return 2;
}
