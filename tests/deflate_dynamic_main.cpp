// deflate_dynamic_main.cpp -- level 2 of the host part of m6anet_amd/csrc/m6a_deflate.h as a program of its own, for the sanitizers
// (tests/test_deflate_dynamic_core.py builds it with -fsanitize=address,undefined and runs it as a child process).
//
//   deflate_dynamic lengths
//       code_lengths on its own, from heap allocations of exactly the sizes it is promised: Fibonacci counts over 2..40 symbols at
//       the limits 7 and 15, equal counts over 1, 2, 3, 19, 30 and 286 symbols, one symbol, none, and 286 counts of 1 beside one of
//       65 000.  One line per case: `<name>\t<limit>\t<counts, comma-separated>\t<lengths, comma-separated>`.
//   deflate_dynamic FILE...
//       every file at both levels as tests/deflate_core_main.cpp does it at level 1: block by block from allocations of exactly the
//       text's length, twice (into a slot, then into exactly the size the first run gave), decoded again by the core of m6a_bgzf.h.
//       A level-2 block must not be larger than the level-1 block.  Two lines per file:
//       `<path>\t<level>\t<bytes of BGZF, marker included>\t<crc32 of them>\t<stored>\t<fixed>\t<dynamic>\t<depth>\t<used>`, where
//       depth is that of an unlimited Huffman code of the first block's literal/length counts and used the number of those counts
//       that are not zero.  A file named `fibonacci` whose depth is not over 15 ends the program with status 3.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "m6a_deflate.h"

namespace {

using namespace m6a_deflate;

bool read_file(const char *path, std::vector<uint8_t> &d)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t got;
    d.clear();
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(f);
    return true;
}

void lengths_case(const char *name, const std::vector<uint32_t> &counts, int limit)
{
    const size_t n = counts.size();
    std::unique_ptr<uint32_t[]> freq(new uint32_t[n]), work(new uint32_t[2 * n]);
    std::unique_ptr<uint8_t[]> out(new uint8_t[n]);
    for (size_t i = 0; i < n; i++) freq[i] = counts[i];
    memset(out.get(), 0xee, n);
    code_lengths(freq.get(), (int)n, limit, out.get(), work.get());
    printf("%s\t%d\t", name, limit);
    for (size_t i = 0; i < n; i++) printf("%s%u", i ? "," : "", counts[i]);
    printf("\t");
    for (size_t i = 0; i < n; i++) printf("%s%d", i ? "," : "", out[i]);
    printf("\n");
}

int lengths_main()
{
    for (int limit : {7, 15})
        for (int n = 2; n <= 40; n++) {
            std::vector<uint32_t> f{1, 1};
            while ((int)f.size() < n) f.push_back(f[f.size() - 1] + f[f.size() - 2]);
            // some symbols in between unused, and not in ascending order: symbol i has the count of rank (7 i) mod n
            std::vector<uint32_t> g;
            for (int i = 0; i < n; i++) {
                g.push_back(f[(size_t)(7 * i % n)]);
                if (i % 5 == 2) g.push_back(0);
            }
            lengths_case(("fibonacci_" + std::to_string(n)).c_str(), n % 7 ? g : f, limit);
        }
    for (int n : {1, 2, 3, 19, 30, 286}) {
        lengths_case(("equal_" + std::to_string(n)).c_str(), std::vector<uint32_t>((size_t)n, 5), n == 19 ? 7 : 15);
    }
    std::vector<uint32_t> one(30, 0);
    one[17] = 123;
    lengths_case("one_symbol", one, 15);
    lengths_case("no_symbol", std::vector<uint32_t>(30, 0), 15);
    lengths_case("no_symbol_at_all", std::vector<uint32_t>(), 15);
    std::vector<uint32_t> big(286, 1);
    big[256] = 65000;
    lengths_case("ones_and_65000", big, 15);
    return 0;
}

// the depth of the deepest leaf of a Huffman tree of the counts that are not zero (of two equal weights the shallower is merged first)
int huffman_depth(const uint32_t *freq, int n)
{
    std::vector<std::pair<uint64_t, int>> node;
    for (int i = 0; i < n; i++)
        if (freq[i]) node.push_back({freq[i], 0});
    if (node.size() < 2) return (int)node.size();
    while (node.size() > 1) {
        size_t a = 0, b = 1;
        if (node[b] < node[a]) std::swap(a, b);
        for (size_t i = 2; i < node.size(); i++) {
            if (node[i] < node[a]) { b = a; a = i; }
            else if (node[i] < node[b]) b = i;
        }
        const std::pair<uint64_t, int> m{node[a].first + node[b].first, std::max(node[a].second, node[b].second) + 1};
        node.erase(node.begin() + (long)std::max(a, b));
        node.erase(node.begin() + (long)std::min(a, b));
        node.push_back(m);
    }
    return node[0].second;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "lengths")) return lengths_main();
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; i++) tab[i] = m6a_bgzf::crc_entry(i);
    std::unique_ptr<uint16_t[]> table(new uint16_t[kTableEntries]);
    std::unique_ptr<m6a_bgzf::Tables> T(new m6a_bgzf::Tables);
    std::vector<uint8_t> d;
    int status = 0;
    for (int a = 1; a < argc; a++) {
        if (!read_file(argv[a], d)) {
            printf("%s\tcannot read\n", argv[a]);
            return 2;
        }
        const int64_t n = (int64_t)d.size();
        int depth = 0, used = 0;
        if (n) {                                             // the first block's counts, as block_host takes them
            const int32_t len = (int32_t)(n < kBlockInput ? n : kBlockInput);
            std::unique_ptr<uint8_t[]> in(new uint8_t[(size_t)len]);
            memcpy(in.get(), d.data(), (size_t)len);
            uint32_t freq[kSymbols] = {0}, bits, head, extra;
            for (int lane = 0; lane < kParts; lane++) part_hist<PlainAdd>(in.get(), len, lane, table.get(), freq, &bits, &head, &extra);
            depth = huffman_depth(freq, kLitLen);
            for (int s = 0; s < kLitLen; s++) used += freq[s] != 0;
        }
        std::vector<int32_t> level1;
        for (int level = 1; level <= 2; level++) {
            int64_t total = 0, by_type[3] = {0, 0, 0}, nb = 0;
            uint32_t crc_all = 0xffffffffu;
            const char *wrong = nullptr;
            auto take = [&](const uint8_t *p, int64_t k) {
                for (int64_t i = 0; i < k; i++) crc_all = tab[(crc_all ^ p[i]) & 0xff] ^ (crc_all >> 8);
                total += k;
            };
            for (int64_t off = 0; off < n && !wrong; off += kBlockInput, nb++) {
                const int32_t len = (int32_t)(n - off < kBlockInput ? n - off : kBlockInput);
                std::unique_ptr<uint8_t[]> in(new uint8_t[(size_t)len]), slot(new uint8_t[kSlot]);
                memcpy(in.get(), d.data() + off, (size_t)len);
                int btype = -1, again = -1;
                const int32_t size = block_host(in.get(), len, slot.get(), table.get(), tab, level, &btype);
                if (size < kHeader + kFooter || size > kSlot) { wrong = "a block outside 26..65536 bytes"; break; }
                if (btype < 0 || btype > level) { wrong = "a block type the level does not write"; break; }
                std::unique_ptr<uint8_t[]> blk(new uint8_t[(size_t)size]);
                if (block_host(in.get(), len, blk.get(), table.get(), tab, level, &again) != size || again != btype ||
                    memcmp(blk.get(), slot.get(), (size_t)size) != 0) { wrong = "the second run differs from the first"; break; }
                if (level == 1) level1.push_back(size);
                else if (size > level1[(size_t)nb]) { wrong = "a level-2 block larger than the level-1 block"; break; }
                int32_t tot = 0, hdr = 0;
                if (m6a_bgzf::block_header(blk.get(), size, &tot, &hdr) != 0 || tot != size || hdr != kHeader) { wrong = "bad header"; break; }
                if (m6a_bgzf::le32(blk.get() + size - 4) != (uint32_t)len) { wrong = "ISIZE is not the text's length"; break; }
                if (((blk[(size_t)hdr] >> 1) & 3) != btype || !(blk[(size_t)hdr] & 1)) { wrong = "the first three bits are not BFINAL and the type"; break; }
                std::unique_ptr<uint8_t[]> body(new uint8_t[(size_t)(size - hdr - 8)]), out(new uint8_t[(size_t)len]);
                memcpy(body.get(), blk.get() + hdr, (size_t)(size - hdr - 8));
                m6a_bgzf::HostOut o{out.get()};
                if (m6a_bgzf::inflate(body.get(), size - hdr - 8, o, len, *T) != 0) { wrong = "the decode core refuses the stream"; break; }
                if (memcmp(out.get(), in.get(), (size_t)len) != 0) { wrong = "the inflated block is not the text"; break; }
                uint32_t c = 0;
                for (int lane = 0; lane < 64; lane++) c ^= m6a_bgzf::crc_lane(tab, out.get(), len, lane);
                if (c != m6a_bgzf::le32(blk.get() + size - 8)) { wrong = "CRC-32 mismatch"; break; }
                by_type[btype]++;
                take(blk.get(), size);
            }
            if (wrong) {
                printf("%s\t%d\t%s\n", argv[a], level, wrong);
                return 1;
            }
            uint8_t eof[kEofBytes];
            for (int i = 0; i < kEofBytes; i++) eof[i] = eof_byte(i);
            take(eof, kEofBytes);
            printf("%s\t%d\t%lld\t%08x\t%lld\t%lld\t%lld\t%d\t%d\n", argv[a], level, (long long)total, ~crc_all, (long long)by_type[0],
                   (long long)by_type[1], (long long)by_type[2], depth, used);
        }
        if (!strcmp(argv[a], "fibonacci") && depth <= kMaxBits) status = 3;
    }
    return status;
}
