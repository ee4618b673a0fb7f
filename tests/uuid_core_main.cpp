// The read-name core (m6anet_amd/csrc/m6a_uuid.h) as a program of its own: tests/test_read_names_core.py builds it with ASan and UBSan
// and compares what it prints with tests/read_names_statement.py.  Every field is copied into an allocation of exactly its size
// first, so a read at or past `end` is a sanitizer report.
//   fields FILE     a field per line -> its 128 bits as 32 hex digits, a blank and the 36 bytes format() makes of them, or "refused"
//   cuts FILE       a text per line -> a letter per length 0..strlen: 'a' where its first bytes of that length are a name, else 'r'
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>

#include "m6a_uuid.h"

static bool parse_exact(const std::string &s, size_t len, m6a_uuid::Name *out)
{
    std::unique_ptr<uint8_t[]> buf(new uint8_t[len]);       // len 0: a valid pointer to nothing
    if (len) memcpy(buf.get(), s.data(), len);
    return m6a_uuid::parse(buf.get(), buf.get() + len, out);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const std::string mode = argv[1];
    std::ifstream in(argv[2], std::ios::binary);
    if (!in) return 2;
    std::string line;
    while (std::getline(in, line)) {
        if (mode == "fields") {
            m6a_uuid::Name nm{0, 0};
            if (!parse_exact(line, line.size(), &nm)) { puts("refused"); continue; }
            std::unique_ptr<char[]> text(new char[m6a_uuid::kLen]);
            m6a_uuid::format(nm.hi, nm.lo, text.get());
            uint8_t raw[16];
            m6a_uuid::to_bytes(nm.hi, nm.lo, raw);
            const m6a_uuid::Name back = m6a_uuid::from_bytes(raw);
            if (back.hi != nm.hi || back.lo != nm.lo) return 3;
            printf("%016" PRIx64 "%016" PRIx64 " %.*s\n", nm.hi, nm.lo, m6a_uuid::kLen, text.get());
        } else if (mode == "cuts") {
            std::string out;
            for (size_t len = 0; len <= line.size(); len++) {
                m6a_uuid::Name nm{0, 0};
                out += parse_exact(line, len, &nm) ? 'a' : 'r';
            }
            puts(out.c_str());
        } else return 2;
    }
    return 0;
}
