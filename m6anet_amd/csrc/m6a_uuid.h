// m6a_uuid.h -- a read name as nanopolish / f5c --print-read-names write it: 36 bytes, 8-4-4-4-12 lowercase hex digits with '-' at
// offsets 8, 13, 18 and 23 -- 128 bits, and it prints back as the same bytes.  Plain C++ marked for host and device: m6a_prep.hip
// compiles it for gfx950 (line_kernel reads field 4 with it, the CSV kernels print with it), m6a_io.cpp compiles it for the CPU
// (m6a_io_uuid_parse / m6a_io_uuid_format, the host CSV writer), and tests/uuid_core_main.cpp holds it to
// tests/read_names_statement.py as a program of its own under ASan and UBSan.
//   parse    the field is [p, end): accepted when it is exactly 36 bytes of that shape.  Anything else -- upper case, 35 or 37
//            bytes, a dash elsewhere, a plain integer, nothing -- is refused.  No byte at or past `end` is read.
//   format   hi, lo -> 36 bytes, no terminator.
#ifndef M6A_UUID_H
#define M6A_UUID_H
#include <stdint.h>

#ifndef M6A_HD
#if defined(__HIPCC__)
#define M6A_HD __host__ __device__
#else
#define M6A_HD
#endif
#endif

namespace m6a_uuid {

constexpr int kLen = 36;

struct Name { uint64_t hi, lo; };          // the 32 hex digits as one 128-bit number, the first digit the most significant

M6A_HD inline bool parse(const uint8_t *p, const uint8_t *end, Name *out)
{
    if (end - p != kLen) return false;
    uint64_t w[2] = {0, 0};
    int nd = 0;
    for (int i = 0; i < kLen; i++) {
        const unsigned c = p[i];
        if (i == 8 || i == 13 || i == 18 || i == 23) {
            if (c != '-') return false;
            continue;
        }
        unsigned d;
        if (c - '0' < 10u) d = c - '0';
        else if (c - 'a' < 6u) d = c - 'a' + 10;
        else return false;
        w[nd >> 4] = w[nd >> 4] << 4 | d;
        ++nd;
    }
    out->hi = w[0];
    out->lo = w[1];
    return true;
}

M6A_HD inline void format(uint64_t hi, uint64_t lo, char *o)
{
    int nd = 0;
    for (int i = 0; i < kLen; i++) {
        if (i == 8 || i == 13 || i == 18 || i == 23) { o[i] = '-'; continue; }
        const unsigned d = (unsigned)((nd < 16 ? hi >> (60 - 4 * nd) : lo >> (60 - 4 * (nd - 16))) & 15);
        o[i] = (char)(d < 10 ? '0' + d : 'a' + (d - 10));
        ++nd;
    }
}

// the table's form: 16 bytes per name, hi then lo, most significant byte first -- the UUID's own byte order
M6A_HD inline void to_bytes(uint64_t hi, uint64_t lo, uint8_t *o)
{
    for (int k = 0; k < 8; k++) { o[k] = (uint8_t)(hi >> (56 - 8 * k)); o[8 + k] = (uint8_t)(lo >> (56 - 8 * k)); }
}

M6A_HD inline Name from_bytes(const uint8_t *b)
{
    Name n{0, 0};
    for (int k = 0; k < 8; k++) { n.hi = n.hi << 8 | b[k]; n.lo = n.lo << 8 | b[8 + k]; }
    return n;
}

}  // namespace m6a_uuid
#endif
