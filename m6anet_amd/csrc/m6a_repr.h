// m6a_repr.h -- the numbers of data.json, eventalign.index and data.info as text.  Plain C++ marked for host and device:
// m6a_prep.hip compiles it for gfx950 (m6a_dataprep.h: the kernels behind `dataprep --device gpu --writer device` and
// m6a_repr_format), m6a_io.cpp compiles it for the CPU (m6a_io_repr_core), and tests/repr_core_main.cpp holds it to Python's repr
// as a program of its own under ASan and UBSan.
//   repr      Python's repr(float) -- what py_repr in m6a_io.cpp gives through std::to_chars -- for exactly the finite v with
//             1e-4 <= v < 1e16: the shortest digits that round-trip, written positionally, `.0` on an integral value, at most
//             kMaxLen bytes, no terminator.  Everything else -- zero, negatives, below 1e-4, 1e16 and above, NaN, the infinities
//             -- is DECLINED: -1, nothing written.
//             v = m 2^e with 2^52 <= m < 2^53 and -66 <= e <= 1 in that range.  e >= 0: v is an integer below 1e16 and its neighbours
//             are 2 away, so no shorter decimal rounds to it: the integer and `.0`.  e < 0: the integer part is m >> -e (half an
//             ulp is at most 1/4, so every digit of it is needed), and the fraction is generated digit by digit in exact integer
//             arithmetic (Steele & White's free-format generation with Burger & Dybvig's bounds): R, the remainder, and the half
//             gaps below and above v are kept in units of 2^(e-2), ten times larger with every digit; the scale S = 2^(2-e) is a power
//             of two, so a digit is a shift and the remainder a mask.  Generation stops at the first digit after which the rest can
//             be dropped (R within the gap below) or rounded up (R + gap above reaches S) without leaving the interval that rounds
//             to v -- closed when m is even, as round-half-even makes it; the gap below is half as wide when m = 2^52 -- and of the
//             two the nearer one is taken.  The rounded-up digit is never 10: that decimal would have ended the loop one digit
//             earlier.  A tie between the two would need an odd multiple of 5 10^-(n+1) that is a multiple of 2^e >= 10^-n: there
//             is none.  R 10 < 2^72: 128-bit integers, no table.
//   np_round  np.round(v, 3) as the host writer computes it for --compress: nearbyint(v * 1000) / 1000, two IEEE operations (the
//             translation units are built with -ffp-contract=off or for a CPU without fusing across statements)
//   i64       a signed 64-bit integer in decimal: positions, offsets, counts
//   read_id   repr(float(read)) of a read index: `<digits>.0` for 0 <= read < 2^53, declined (-1) otherwise
#ifndef M6A_REPR_H
#define M6A_REPR_H
#include <math.h>
#include <stdint.h>

#ifndef M6A_HD
#if defined(__HIPCC__)
#define M6A_HD __host__ __device__
#else
#define M6A_HD
#endif
#endif

namespace m6a_repr {

constexpr int kMaxLen = 24;                 // the longest repr() taken: 0.000ddddddddddddddddd is 22

M6A_HD inline int u64_digits(uint64_t v)
{
    int n = 1;
    for (uint64_t p = 10; n < 20 && v >= p; p *= 10) ++n;
    return n;
}

// PUT = false everywhere below: the length alone, `o` is not touched
template <bool PUT>
M6A_HD inline int u64(uint64_t v, char *o)
{
    const int nd = u64_digits(v);
    if (PUT)
        for (int i = nd; i > 0;) { const uint64_t q = v / 10; o[--i] = (char)('0' + (int)(v - q * 10)); v = q; }
    return nd;
}

template <bool PUT>
M6A_HD inline int i64(int64_t v, char *o)
{
    uint64_t u = (uint64_t)v;
    int k = 0;
    if (v < 0) { if (PUT) o[0] = '-'; k = 1; u = 0 - u; }
    return k + u64<PUT>(u, o + k);
}

template <bool PUT>
M6A_HD inline int read_id(int64_t read, char *o)
{
    if (read < 0 || read >= (int64_t)1 << 53) return -1;
    const int n = u64<PUT>((uint64_t)read, o);
    if (PUT) { o[n] = '.'; o[n + 1] = '0'; }
    return n + 2;
}

M6A_HD inline double np_round3(double v) { return nearbyint(v * 1000.0) / 1000.0; }

M6A_HD inline bool takes(double v) { return v >= 1e-4 && v < 1e16; }          // false for NaN

template <bool PUT>
M6A_HD inline int repr(double v, char *o)
{
    if (!takes(v)) return -1;
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    const uint64_t frac = b & ((1ull << 52) - 1), m = frac | 1ull << 52;
    const int e = ((int)(b >> 52) & 0x7ff) - 1075;          // -66 .. 1
    if (e >= 0) {
        const int n = u64<PUT>(m << e, o);
        if (PUT) { o[n] = '.'; o[n + 1] = '0'; }
        return n + 2;
    }
    const int k = -e, sh = k + 2;                            // sh <= 68
    int n = u64<PUT>(k < 64 ? m >> k : 0, o);
    if (PUT) o[n] = '.';
    ++n;
    typedef unsigned __int128 u128;
    const u128 S = (u128)1 << sh;
    u128 R = ((u128)m << 2) & (S - 1), up = 2, down = frac ? 2 : 1;
    if (R == 0) {
        if (PUT) o[n] = '0';
        return n + 1;
    }
    const bool even = !(m & 1);
    for (;;) {
        R *= 10; up *= 10; down *= 10;
        int d = (int)(R >> sh);
        R &= S - 1;
        const bool low = even ? R <= down : R < down, high = even ? R + up >= S : R + up > S;
        if (low || high) {
            if (high && (!low || 2 * R > S || (2 * R == S && (d & 1)))) ++d;
            if (PUT) o[n] = (char)('0' + d);
            return n + 1;
        }
        if (PUT) o[n] = (char)('0' + d);
        ++n;
    }
}

// one number of data.json: np.round(v, 3) first under --compress
template <bool PUT>
M6A_HD inline int feature(double v, int round3, char *o) { return repr<PUT>(round3 ? np_round3(v) : v, o); }

}  // namespace m6a_repr
#endif
