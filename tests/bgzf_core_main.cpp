// bgzf_core_main.cpp -- the host part of m6anet_amd/csrc/m6a_bgzf.h as a program of its own, for the sanitizers
// (tests/test_bgzf_generated.py builds it with -fsanitize=address,undefined and runs it as a child process).
//
// For every file named on the command line: the block chain is walked with the file fed to Walker in pieces of each size below,
// every piece in a heap allocation of exactly its length, and the block list, `bad`, `bad_at` and `next` must be those of the
// one-piece walk.  Then every block is inflated from a buffer of exactly its stream's length into a buffer of exactly ISIZE bytes, so
// a byte touched outside either is a sanitizer report, and its CRC is formed from the 64 lane terms as bgzf_crc_kernel forms it.
// One line per file: `<path>\tok\t<bytes of text>\t<crc32 of the text>` or `<path>\t<offset of the first bad block>\t<reason>`.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "m6a_bgzf.h"

namespace {

using namespace m6a_bgzf;

struct Blk {
    int64_t at;
    int32_t hdr, total;
    uint32_t crc;
    int32_t isize;
    bool operator==(const Blk &o) const { return at == o.at && hdr == o.hdr && total == o.total && crc == o.crc && isize == o.isize; }
};
struct Walk {
    std::vector<Blk> blocks;
    int bad = 0;
    int64_t bad_at = 0, next = 0;
    bool operator==(const Walk &o) const { return blocks == o.blocks && bad == o.bad && bad_at == o.bad_at && next == o.next; }
};

Walk walk(const std::vector<uint8_t> &d, int64_t piece)     // piece 0: the whole file
{
    Walk r;
    auto on_block = [&](int64_t off, int32_t hdr, int32_t tot, uint32_t crc, int32_t isize) { r.blocks.push_back(Blk{off, hdr, tot, crc, isize}); };
    std::unique_ptr<Walker<decltype(on_block)>> W(new Walker<decltype(on_block)>(on_block));
    const int64_t n = (int64_t)d.size();
    if (piece <= 0) piece = n > 0 ? n : 1;
    for (int64_t off = 0; off < n; off += piece) {
        const int64_t len = piece < n - off ? piece : n - off;
        std::unique_ptr<uint8_t[]> p(new uint8_t[(size_t)len]);
        memcpy(p.get(), d.data() + off, (size_t)len);
        W->feed(p.get(), len);
    }
    W->finish();
    r.bad = W->bad;
    r.bad_at = W->bad_at;
    r.next = W->next;
    return r;
}

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

}  // namespace

int main(int argc, char **argv)
{
    std::vector<int64_t> pieces = {1, 2, 3, 5, 7, 11, 12, 13, 17, 18, 19, 26, 28, 29, 64, 97, 4096, 65535, 65536};
    for (int k = 1; k <= 40; k++) pieces.push_back(4096 - k);
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; i++) tab[i] = crc_entry(i);
    std::unique_ptr<Tables> T(new Tables);
    std::vector<uint8_t> d;
    for (int a = 1; a < argc; a++) {
        if (!read_file(argv[a], d)) {
            printf("%s\tcannot read\n", argv[a]);
            return 2;
        }
        const Walk whole = walk(d, 0);
        for (int64_t piece : pieces)
            if (!(walk(d, piece) == whole)) {
                printf("%s\tthe walk in pieces of %lld bytes is not the walk of the whole file\n", argv[a], (long long)piece);
                return 1;
            }
        int reason = 0;
        int64_t at = 0, n_text = 0;
        uint32_t crc_text = 0xffffffffu;
        for (const Blk &b : whole.blocks) {
            const int32_t n = b.total - b.hdr - 8;
            std::unique_ptr<uint8_t[]> in(new uint8_t[(size_t)n]), out(new uint8_t[(size_t)b.isize]);
            memcpy(in.get(), d.data() + b.at + b.hdr, (size_t)n);
            HostOut o{out.get()};
            int r = inflate(in.get(), n, o, b.isize, *T);
            if (!r) {
                uint32_t c = 0;
                for (int lane = 0; lane < 64; lane++) c ^= crc_lane(tab, out.get(), b.isize, lane);
                if (c != b.crc) r = BR_CRC;
            }
            if (r) {
                reason = r;
                at = b.at;
                break;
            }
            for (int32_t i = 0; i < b.isize; i++) crc_text = tab[(crc_text ^ out[(size_t)i]) & 0xff] ^ (crc_text >> 8);
            n_text += b.isize;
        }
        if (!reason && whole.bad) {
            reason = whole.bad;
            at = whole.bad_at;
        }
        if (reason) printf("%s\t%lld\t%s\n", argv[a], (long long)at, reason_text(reason));
        else printf("%s\tok\t%lld\t%08x\n", argv[a], (long long)n_text, ~crc_text);
    }
    return 0;
}
