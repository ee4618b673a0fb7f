// deflate_core_main.cpp -- the host part of m6anet_amd/csrc/m6a_deflate.h as a program of its own, for the sanitizers
// (tests/test_deflate_core.py builds it with -fsanitize=address,undefined and runs it as a child process).
//
// For every file named on the command line: its bytes are cut into blocks of 65 280; every block is deflated from a heap allocation
// of exactly its length, once into a 64 KiB slot and once more into an allocation of exactly the size the first run returned, so a
// byte touched outside the text or the block is a sanitizer report; the two runs must give the same bytes.  The block is then read
// back by the decode core of m6a_bgzf.h (header, inflate, CRC-32 from the 64 lane terms) and must give the text.
// One line per file: `<path>\t<bytes of BGZF, marker included>\t<crc32 of them>\t<stored blocks>`, or `<path>\t<what went wrong>`.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "m6a_deflate.h"

namespace {

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
    using namespace m6a_deflate;
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; i++) tab[i] = m6a_bgzf::crc_entry(i);
    std::unique_ptr<uint16_t[]> table(new uint16_t[kTableEntries]);
    std::unique_ptr<m6a_bgzf::Tables> T(new m6a_bgzf::Tables);
    std::vector<uint8_t> d;
    for (int a = 1; a < argc; a++) {
        if (!read_file(argv[a], d)) {
            printf("%s\tcannot read\n", argv[a]);
            return 2;
        }
        const int64_t n = (int64_t)d.size();
        int64_t total = 0, n_stored = 0;
        uint32_t crc_all = 0xffffffffu;
        const char *wrong = nullptr;
        auto take = [&](const uint8_t *p, int64_t k) {
            for (int64_t i = 0; i < k; i++) crc_all = tab[(crc_all ^ p[i]) & 0xff] ^ (crc_all >> 8);
            total += k;
        };
        for (int64_t off = 0; off < n && !wrong; off += kBlockInput) {
            const int32_t len = (int32_t)(n - off < kBlockInput ? n - off : kBlockInput);
            std::unique_ptr<uint8_t[]> in(new uint8_t[(size_t)len]), slot(new uint8_t[kSlot]);
            memcpy(in.get(), d.data() + off, (size_t)len);
            bool stored = false, again = false;
            const int32_t size = block_host(in.get(), len, slot.get(), table.get(), tab, &stored);
            if (size < kHeader + kFooter || size > kSlot) { wrong = "a block outside 26..65536 bytes"; break; }
            std::unique_ptr<uint8_t[]> blk(new uint8_t[(size_t)size]);
            if (block_host(in.get(), len, blk.get(), table.get(), tab, &again) != size || again != stored ||
                memcmp(blk.get(), slot.get(), (size_t)size) != 0) { wrong = "the second run differs from the first"; break; }
            int32_t tot = 0, hdr = 0;
            if (m6a_bgzf::block_header(blk.get(), size, &tot, &hdr) != 0 || tot != size || hdr != kHeader) { wrong = "bad header"; break; }
            if (m6a_bgzf::le32(blk.get() + size - 4) != (uint32_t)len) { wrong = "ISIZE is not the text's length"; break; }
            std::unique_ptr<uint8_t[]> body(new uint8_t[(size_t)(size - hdr - 8)]), out(new uint8_t[(size_t)len]);
            memcpy(body.get(), blk.get() + hdr, (size_t)(size - hdr - 8));
            m6a_bgzf::HostOut o{out.get()};
            if (m6a_bgzf::inflate(body.get(), size - hdr - 8, o, len, *T) != 0) { wrong = "the decode core refuses the stream"; break; }
            if (memcmp(out.get(), in.get(), (size_t)len) != 0) { wrong = "the inflated block is not the text"; break; }
            uint32_t c = 0;
            for (int lane = 0; lane < 64; lane++) c ^= m6a_bgzf::crc_lane(tab, out.get(), len, lane);
            if (c != m6a_bgzf::le32(blk.get() + size - 8)) { wrong = "CRC-32 mismatch"; break; }
            n_stored += stored;
            take(blk.get(), size);
        }
        if (wrong) {
            printf("%s\t%s\n", argv[a], wrong);
            return 1;
        }
        uint8_t eof[kEofBytes];
        for (int i = 0; i < kEofBytes; i++) eof[i] = eof_byte(i);
        take(eof, kEofBytes);
        printf("%s\t%lld\t%08x\t%lld\n", argv[a], (long long)total, ~crc_all, (long long)n_stored);
    }
    return 0;
}
