// m6a_json.h -- data.json read for `inference --loader device` (include/m6a.h states the format at m6a_json_sites_build).
//
// Part 1, the decode core: the decimal -> double conversion, the record grammar and every check, as plain C++ marked for host and
// device.  m6a_io.cpp compiles it for the CPU (m6a_io_json_walk), tests/json_core_main.cpp holds it to
// tests/json_statement.py as a program of its own under ASan and UBSan, and m6a_prep.hip compiles the same text for gfx950.
//   number   an ACCEPTED token is an optional '-', digits with at most one '.', at least one digit, at most 19 significant digits
//            (from the first non-zero digit on, trailing zeros included) and at most 27 digits behind the point, followed by a byte
//            that is none of [0-9A-Za-z+-.].  Its value w / 10^k (w < 10^19 < 2^64) is rounded to nearest, ties to even, exactly:
//              w < 2^53 and k <= 22   (double)w / 10^k -- both exact doubles, one IEEE division (Clinger);
//              otherwise              w / 5^k as the 64-bit quotient of the two normalised integers (5^27 < 2^63) with the remainder
//                                     as a sticky bit, rounded to 53 bits, scaled by a power of two; no result is subnormal.
//            There is no third path.  Everything else -- an exponent, '+', a name, 20 digits, a second '.' -- is not accepted, and
//            the site that holds it is declined.
//   record   {"<tx>":{"<pos>":{"<7-mer>":[[n x 10],...]}}} with the loader's whitespace set between tokens and nothing but
//            whitespace behind it.  Every read is `p < e` checked; a caller's sink writes row r only while r < n_reads.
// A site the core does not take is a reason code (JR_*), never an error: m6a_io_info_rows parses it again on the host and either
// returns its rows or the loader's own error.
//
// Part 2 (M6A_JSON_DEVICE_PART, m6a_prep.hip only): the kernels and m6a_json_sites_build.
//   json_scan_kernel   one wave per site.  Every lane walks the header (the same bytes: the loads are broadcasts); the norm and
//                      vocabulary lookups of the three 5-mers follow.  Then each lane takes 16 bytes of the body at a time (an aligned
//                      16-byte load, bytes outside [body, end) masked), the '[' counts are prefix-summed over the wave, and the offset of
//                      row r goes to row_start[off[s] + r] while r < n_reads.  A count other than n_reads declines the site.
//   json_rows_kernel   one wave per site the first kernel took, a lane per row, rows lane, lane + 64, ...: ten numbers, X and the read
//                      id written, and the bytes behind the row must lead to the next row's start (the last row's to the end of the
//                      record).  A site of 5 000 reads is 79 rounds of one wave; nothing is staged in LDS, so no site is too large.
//   status             one byte per site, 0 or the reason; it and the read ids are all that comes back per site and per read.
#ifndef M6A_JSON_H
#define M6A_JSON_H
#include <stdint.h>
#include <string.h>

#ifndef M6A_HD
#if defined(__HIPCC__)
#define M6A_HD __host__ __device__
#else
#define M6A_HD
#endif
#endif

namespace m6a_json {

// reasons, in the order the walk meets them; the names are those of tests/json_statement.py
enum {
    JR_OK = 0, JR_RANGE, JR_JSON, JR_TX, JR_POS, JR_KEY, JR_EMPTY, JR_ROW, JR_NUMBER, JR_COLS, JR_TAIL, JR_KEYS, JR_COUNT, JR_NORM, JR_VOCAB,
    JR_N
};
inline const char *reason_name(int r)
{
    static const char *const t[JR_N] = {"ok", "range", "json", "transcript", "position", "key", "empty", "row", "number", "columns", "tail",
                                        "keys", "count", "norm", "vocabulary"};
    return r >= 0 && r < JR_N ? t[r] : "?";
}
constexpr int JR_CLOSED = -1;               // after_row: the row list and the record ended well

constexpr int kMaxDigits = 19, kMaxFrac = 27;

M6A_HD inline bool is_ws(unsigned c) { return c == ' ' || c == '\n' || c == '\r' || c == '\t'; }
M6A_HD inline const uint8_t *skip_ws(const uint8_t *p, const uint8_t *e)
{
    while (p < e && is_ws(*p)) ++p;
    return p;
}
// a byte that would make a longer token of the digits in front of it
M6A_HD inline bool is_token_byte(unsigned c)
{
    return c - '0' <= 9u || (c | 32u) - 'a' <= 25u || c == '+' || c == '-' || c == '.';
}

M6A_HD inline double from_bits(uint64_t b)
{
    double d;
    memcpy(&d, &b, 8);
    return d;
}

// 10^k, 0 <= k <= 22: every factor and every product is a power of ten below 10^23, which a double holds exactly
M6A_HD inline double pow10_exact(int k)
{
    double r = 1.0;
    if (k & 1) r *= 1e1;
    if (k & 2) r *= 1e2;
    if (k & 4) r *= 1e4;
    if (k & 8) r *= 1e8;
    if (k & 16) r *= 1e16;
    return r;
}
M6A_HD inline uint64_t pow5_u64(int k)         // 0 <= k <= 27
{
    uint64_t r = 1;
    if (k & 1) r *= 5ull;
    if (k & 2) r *= 25ull;
    if (k & 4) r *= 625ull;
    if (k & 8) r *= 390625ull;
    if (k & 16) r *= 152587890625ull;
    return r;
}

// (u1 * 2^64 + u0) / v for v >= 2^63 and u1 < v: the quotient (below 2^64) and the remainder; Knuth's algorithm D in two 32-bit steps
M6A_HD inline uint64_t div_128_64(uint64_t u1, uint64_t u0, uint64_t v, uint64_t *rem)
{
    const uint64_t b = 1ull << 32, vn1 = v >> 32, vn0 = v & 0xffffffffull, un1 = u0 >> 32, un0 = u0 & 0xffffffffull;
    uint64_t q1 = u1 / vn1, rhat = u1 - q1 * vn1;
    while (q1 >= b || q1 * vn0 > b * rhat + un1) {
        --q1;
        rhat += vn1;
        if (rhat >= b) break;
    }
    const uint64_t un21 = u1 * b + un1 - q1 * v;
    uint64_t q0 = un21 / vn1;
    rhat = un21 - q0 * vn1;
    while (q0 >= b || q0 * vn0 > b * rhat + un0) {
        --q0;
        rhat += vn1;
        if (rhat >= b) break;
    }
    *rem = un21 * b + un0 - q0 * v;
    return q1 * b + q0;
}

// w / 10^k correctly rounded; w < 2^64, 0 <= k <= kMaxFrac
M6A_HD inline double decimal_to_double(uint64_t w, int k)
{
    if (w == 0) return 0.0;
    if (w < (1ull << 53) && k <= 22) return (double)(int64_t)w / pow10_exact(k);
    const uint64_t d = pow5_u64(k);
    const int lw = __builtin_clzll(w), ld = __builtin_clzll(d);
    const uint64_t wn = w << lw, dn = d << ld;         // both in [2^63, 2^64): wn / dn in (1/2, 2)
    uint64_t rem;
    const uint64_t q = div_128_64(wn >> 1, wn << 63, dn, &rem);      // floor(wn * 2^63 / dn) in [2^62, 2^64)
    const int drop = 11 - __builtin_clzll(q);                        // 64 - clz - 53: 10 or 11 bits go
    uint64_t m = q >> drop;
    const uint64_t low = q & ((1ull << drop) - 1), half = 1ull << (drop - 1);
    if (low > half || (low == half && (rem != 0 || (m & 1)))) ++m;
    // w / 10^k = (q + fraction) * 2^(ld - lw - k - 63)
    const int ex = drop + ld - lw - k - 63;                          // -165 .. 11: the scale is a normal double
    return (double)(int64_t)m * from_bits((uint64_t)(1023 + ex) << 52);
}

// the token at p: the byte behind it and its value, or NULL when it is not accepted
M6A_HD inline const uint8_t *number(const uint8_t *p, const uint8_t *e, double *out)
{
    bool neg = false;
    if (p < e && *p == '-') { neg = true; ++p; }
    uint64_t w = 0;
    int nd = 0, frac = 0;
    bool dot = false, any = false;
    for (; p < e; ++p) {
        const unsigned c = *p;
        if (c - '0' <= 9u) {
            any = true;
            if (w != 0 || c != '0') {
                if (++nd > kMaxDigits) return nullptr;
                w = w * 10 + (c - '0');
            }
            if (dot && ++frac > kMaxFrac) return nullptr;
        } else if (c == '.' && !dot) {
            dot = true;
        } else {
            break;
        }
    }
    if (!any || (p < e && is_token_byte(*p))) return nullptr;
    const double v = decimal_to_double(w, frac);
    *out = neg ? -v : v;
    return p;
}

// a string at p (after whitespace): its bytes [*s, *s + *n) as the loader takes them -- raw, a backslash skipping the byte behind it
M6A_HD inline const uint8_t *string(const uint8_t *p, const uint8_t *e, const uint8_t **s, int64_t *n, bool *backslash)
{
    p = skip_ws(p, e);
    if (p >= e || *p != '"') return nullptr;
    const uint8_t *q = ++p;
    *backslash = false;
    while (p < e && *p != '"') {
        if (*p == '\\') { *backslash = true; ++p; }
        ++p;
    }
    if (p >= e) return nullptr;
    *s = q;
    *n = p - q;
    return p + 1;
}
M6A_HD inline const uint8_t *eat(const uint8_t *p, const uint8_t *e, unsigned c)
{
    p = skip_ws(p, e);
    return p < e && *p == c ? p + 1 : nullptr;
}

// s[0, n) is the decimal of pos as std::to_string writes it
M6A_HD inline bool is_decimal_of(const uint8_t *s, int64_t n, int64_t pos)
{
    const bool neg = n > 0 && s[0] == '-';
    if (neg) { ++s; --n; }
    if (n < 1 || n > 18 || (s[0] == '0' && (n > 1 || neg))) return false;
    int64_t v = 0;
    for (int64_t i = 0; i < n; i++) {
        const unsigned c = (unsigned)s[i] - '0';
        if (c > 9u) return false;
        v = v * 10 + (int64_t)c;
    }
    return (neg ? -v : v) == pos;
}

// {"<tx>":{"<pos>":{"<7-mer>":[   -- *k7 = the 7-mer's bytes, first byte highest; *body = the byte behind the '['
M6A_HD inline int header(const uint8_t *p, const uint8_t *e, const uint8_t *tx, int64_t tx_len, int64_t pos, uint64_t *k7, const uint8_t **body)
{
    const uint8_t *s;
    int64_t n;
    bool bs;
    if (!(p = eat(p, e, '{')) || !(p = string(p, e, &s, &n, &bs)) || !(p = eat(p, e, ':'))) return JR_JSON;
    if (n != tx_len) return JR_TX;
    for (int64_t i = 0; i < n; i++)
        if (s[i] != tx[i]) return JR_TX;
    if (!(p = eat(p, e, '{')) || !(p = string(p, e, &s, &n, &bs)) || !(p = eat(p, e, ':'))) return JR_JSON;
    if (!is_decimal_of(s, n, pos)) return JR_POS;
    if (!(p = eat(p, e, '{')) || !(p = string(p, e, &s, &n, &bs)) || !(p = eat(p, e, ':')) || !(p = eat(p, e, '['))) return JR_JSON;
    if (n != 7 || bs) return JR_KEY;
    uint64_t k = 0;
    for (int i = 0; i < 7; i++) k = k << 8 | s[i];
    *k7 = k;
    *body = p;
    return JR_OK;
}

// the row at p ('[' expected there): sink(j, value) for its ten numbers; *after = the byte behind its ']'
template <class Sink>
M6A_HD inline int row(const uint8_t *p, const uint8_t *e, Sink &&sink, const uint8_t **after)
{
    if (p >= e || *p != '[') return JR_ROW;
    ++p;
    for (int j = 0; j < 10; j++) {
        p = skip_ws(p, e);
        double v;
        const uint8_t *q = number(p, e, &v);
        if (!q) return JR_NUMBER;
        sink(j, v);
        p = skip_ws(q, e);
        if (p >= e || *p != (j < 9 ? ',' : ']')) return JR_COLS;
        ++p;
    }
    *after = p;
    return JR_OK;
}

// behind a row.  JR_OK: a ',' -- *next is where the next row must start; JR_CLOSED: ']' and a good end of the record; else a reason
M6A_HD inline int after_row(const uint8_t *p, const uint8_t *e, const uint8_t **next)
{
    p = skip_ws(p, e);
    if (p < e && *p == ',') {
        *next = skip_ws(p + 1, e);
        return JR_OK;
    }
    if (p >= e || *p != ']') return JR_TAIL;
    p = skip_ws(p + 1, e);
    if (p < e && *p == ',') return JR_KEYS;
    if (!(p = eat(p, e, '}')) || !(p = eat(p, e, '}')) || !(p = eat(p, e, '}'))) return JR_TAIL;
    return skip_ws(p, e) == e ? JR_CLOSED : JR_TAIL;
}

M6A_HD inline uint64_t kmer5_of(uint64_t k7, int c) { return (k7 >> (8 * (2 - c))) & 0xffffffffffull; }      // c = 0, 1, 2
M6A_HD inline int find_key(const uint64_t *keys, int n, uint64_t k)          // sorted, unique; -1 when absent
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo < n && keys[lo] == k ? lo : -1;
}

// One site from its first byte to its last, in order: the statement's walk.  sink(r, j, value) is called for r < n_reads only.
// norm_keys == NULL: no normalisation.  norm_at[3] / vocab_at[3] receive the places of the three 5-mers in the two tables.
template <class Sink>
M6A_HD inline int walk(const uint8_t *p, const uint8_t *e, const uint8_t *tx, int64_t tx_len, int64_t pos, int64_t n_reads, const uint64_t *norm_keys,
                       int n_norm_keys, const uint64_t *vocab_keys, int n_vocab, Sink &&sink, uint64_t *k7, int *norm_at, int *vocab_at)
{
    const uint8_t *q;
    int rc = header(p, e, tx, tx_len, pos, k7, &q);
    if (rc) return rc;
    q = skip_ws(q, e);
    if (q < e && *q == ']') return JR_EMPTY;
    int64_t r = 0;
    for (;;) {
        if (q < e && *q == '[' && r >= n_reads) return JR_COUNT;
        const uint8_t *after;
        if ((rc = row(q, e, [&](int j, double v) { sink(r, j, v); }, &after))) return rc;
        ++r;
        if ((rc = after_row(after, e, &q)) == JR_CLOSED) break;
        if (rc) return rc;
    }
    if (r != n_reads) return JR_COUNT;
    for (int c = 0; c < 3 && norm_keys; c++)
        if ((norm_at[c] = find_key(norm_keys, n_norm_keys, kmer5_of(*k7, c))) < 0) return JR_NORM;
    for (int c = 0; c < 3; c++)
        if ((vocab_at[c] = find_key(vocab_keys, n_vocab, kmer5_of(*k7, c))) < 0) return JR_VOCAB;
    return JR_OK;
}

}  // namespace m6a_json
#endif  // M6A_JSON_H

#if defined(M6A_JSON_DEVICE_PART) && !defined(M6A_JSON_DEVICE_PART_DONE)
#define M6A_JSON_DEVICE_PART_DONE
// ---- part 2: the kernels and m6a_json_sites_build; at the end of m6a_prep.hip; DevMem, Streams, upload_range: m6a_prep_kit.h ----
namespace {

using namespace m6a_json;

struct JsonSite { int64_t start, end, pos; uint32_t tx, pad; };       // end = start = 0: the host found the range outside the file

constexpr int kJsonWaves = kBlk / 64;      // sites per workgroup

// One wave's scan of a site of n rows whose row starts go to row_start[base ..]: the header, then the '[' of the body.  The reason
// (wave-uniform) and the 7-mer; json_scan_kernel and norm_scan_kernel (m6a_norm.h) share it.
__device__ inline int json_scan_site(const uint8_t *__restrict__ f, const JsonSite &st, int64_t base, int64_t n, int lane,
                                     const uint8_t *__restrict__ blob, const int64_t *__restrict__ tx_off, int32_t *__restrict__ row_start,
                                     uint64_t *k7_out)
{
    const uint8_t *const e = f + st.end;
    const uint8_t *body = nullptr;
    uint64_t k7 = 0;
    int reason = JR_RANGE;
    // every lane walks the same header bytes: the result is wave-uniform
    if (st.end > st.start && st.end - st.start < 0x7fffffffll)
        reason = header(f + st.start, e, blob + tx_off[st.tx], tx_off[st.tx + 1] - tx_off[st.tx], st.pos, &k7, &body);
    if (!reason) {
        body = skip_ws(body, e);
        if (body < e && *body == ']') reason = JR_EMPTY;
        else if (n < 1) reason = JR_COUNT;
    }
    if (!reason) {
        const int64_t b0 = body - f, e0 = st.end;
        int64_t cnt = 0;
        bool first_bad = false;
        for (int64_t t0 = b0 & ~(int64_t)15; t0 < e0 && cnt <= n; t0 += 64 * 16) {
            const int64_t t = t0 + lane * 16;
            uint32_t m = 0;
            if (t < e0) {                  // an aligned 16 bytes that begin inside the site: inside the buffer, which is padded to 4 KB
                const uint4 q = *(const uint4 *)(f + t);
                const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const uint32_t c = (wd[i >> 2] >> (8 * (i & 3))) & 0xffu;
                    if (c == '[' && t + i >= b0 && t + i < e0) m |= 1u << i;
                }
            }
            const int c = __popc(m);
            int incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl, d, 64);
                if (lane >= d) incl += o;
            }
            int64_t idx = cnt + incl - c;
            while (m) {
                const int i = __ffs((int)m) - 1;
                m &= m - 1;
                if (idx < n) row_start[base + idx] = (int32_t)(t + i - st.start);      // bounded by the site's n_reads
                if (idx == 0 && t + i != b0) first_bad = true;
                ++idx;
            }
            cnt += __shfl(incl, 63, 64);
        }
        if (cnt != n) reason = JR_COUNT;
        else if (__any(first_bad)) reason = JR_ROW;
    }
    *k7_out = k7;
    return reason;
}

__global__ void __launch_bounds__(kBlk)
json_scan_kernel(const uint8_t *__restrict__ f, const JsonSite *__restrict__ sites, const int64_t *__restrict__ off, int64_t S,
                 const uint8_t *__restrict__ blob, const int64_t *__restrict__ tx_off, const uint64_t *__restrict__ nk,
                 const int32_t *__restrict__ nix, int n_nk, const uint64_t *__restrict__ voc, int n_voc, int32_t *__restrict__ row_start,
                 int32_t *__restrict__ site_norm, uint8_t *__restrict__ site_kmers, uint8_t *__restrict__ site_k7, uint8_t *__restrict__ status)
{
    const int lane = (int)(threadIdx.x & 63);
    const int64_t s = (int64_t)blockIdx.x * kJsonWaves + (threadIdx.x >> 6);
    if (s >= S) return;
    const JsonSite st = sites[s];
    const int64_t base = off[s];
    uint64_t k7 = 0;
    int reason = json_scan_site(f, st, base, off[s + 1] - base, lane, blob, tx_off, row_start, &k7);
    if (!reason) {
        bool no_norm = false, no_voc = false;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint64_t k5 = kmer5_of(k7, c);
            if (n_nk) {
                const int a = find_key(nk, n_nk, k5);
                if (a < 0) no_norm = true;
                else if (lane == 0) site_norm[3 * s + c] = nix[a];
            }
            const int v = find_key(voc, n_voc, k5);
            if (v < 0) no_voc = true;
            else if (lane == 0) site_kmers[3 * s + c] = (uint8_t)v;
        }
        reason = no_norm ? JR_NORM : no_voc ? JR_VOCAB : JR_OK;
    }
    if (lane == 0) {
        status[s] = (uint8_t)reason;
        if (!reason)
            for (int i = 0; i < 7; i++) site_k7[7 * s + i] = (uint8_t)(k7 >> (8 * (6 - i)));
    }
}

struct JsonSink {
    float *x;
    double *id;
    const double *mean, *sd;
    int32_t n0, n1, n2;
    bool norm;
    __device__ void operator()(int j, double v) const
    {
        if (j == 9) { *id = v; return; }
        if (!norm) { x[j] = (float)v; return; }
        const int c = j / 3;
        const int a = 3 * (c == 0 ? n0 : c == 1 ? n1 : n2) + (j - 3 * c);
        x[j] = (float)((v - mean[a]) / sd[a]);
    }
};

// One wave's rows of a site the scan took, a lane per row: sink_of(r) receives row r's ten numbers.  The first reason met by the
// lowest lane that met one (wave-uniform), 0 when every row and what lies between the rows is good; json_rows_kernel and
// norm_rows_kernel (m6a_norm.h) share it.
template <class SinkOf>
__device__ inline int json_rows_site(const uint8_t *__restrict__ f, const JsonSite &st, int64_t base, int64_t n, int lane,
                                     const int32_t *__restrict__ row_start, SinkOf &&sink_of)
{
    const uint8_t *const p0 = f + st.start, *const e = f + st.end;
    int reason = JR_OK;
    for (int64_t r = lane; r < n; r += 64) {
        const auto sink = sink_of(r);
        const uint8_t *after = nullptr, *next = nullptr;
        int rc = row(p0 + row_start[base + r], e, sink, &after);
        if (!rc) {
            rc = after_row(after, e, &next);
            if (r + 1 < n) rc = rc == JR_CLOSED ? JR_COUNT : rc ? rc : next - p0 == row_start[base + r + 1] ? JR_OK : JR_ROW;
            else rc = rc == JR_CLOSED ? JR_OK : rc ? rc : JR_COUNT;
        }
        if (rc && !reason) reason = rc;
    }
    const unsigned long long bad = __ballot(reason != 0);
    return bad ? __shfl(reason, __ffsll((long long)bad) - 1, 64) : JR_OK;
}

__global__ void __launch_bounds__(kBlk)
json_rows_kernel(const uint8_t *__restrict__ f, const JsonSite *__restrict__ sites, const int64_t *__restrict__ off, int64_t S,
                 const int32_t *__restrict__ row_start, const int32_t *__restrict__ site_norm, const double *__restrict__ mean,
                 const double *__restrict__ sd, int n_norm, float *__restrict__ X, double *__restrict__ ids, uint8_t *status)
{
    const int lane = (int)(threadIdx.x & 63);
    const int64_t s = (int64_t)blockIdx.x * kJsonWaves + (threadIdx.x >> 6);
    if (s >= S || status[s]) return;
    const JsonSite st = sites[s];
    const int64_t base = off[s], n = off[s + 1] - base;
    const int32_t n0 = n_norm ? site_norm[3 * s] : 0, n1 = n_norm ? site_norm[3 * s + 1] : 0, n2 = n_norm ? site_norm[3 * s + 2] : 0;
    const int r0 = json_rows_site(f, st, base, n, lane, row_start, [&](int64_t r) {
        return JsonSink{X + 9 * (base + r), ids + base + r, mean, sd, n0, n1, n2, n_norm > 0};
    });
    if (r0 && lane == 0) status[s] = (uint8_t)r0;
}

int json_host_fail(const m6a_json_host_half *host, int hrc)
{
    const int code = hrc == -2 ? M6A_ENOMEM : hrc == -3 ? M6A_EIO : hrc == -4 ? M6A_EFORMAT : hrc == -1 ? M6A_EINVAL : M6A_EIO;
    const std::string text = host->error ? host->error() : "the host half failed";       // copied first: prep_fail formats into its own
    return prep_fail(code, "%s", text.c_str());
}

int json_impl(int device_id, const char *dir, int min_reads, const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm,
              const m6a_json_host_half *host, int n_threads, m6a_prep_sites &P)
{
    const double t_all = now_ms();
    g_d2h = 0;
    double *ms = P.info.ms;
    int rc;

    // ---- the host: data.info through the loader's own parser, the file's size, the site table
    double t1 = now_ms();
    struct Info {
        const m6a_json_host_half *h;
        m6a_io_info *p = nullptr;
        ~Info() { if (p) h->free(p); }
    } info{host};
    int hrc = host->open(dir, min_reads, &info.p);
    if (hrc || !info.p) return json_host_fail(host, hrc);
    const m6a_io_info_table *T = host->table(info.p);
    if (!T) return prep_fail(M6A_EINVAL, "the host half returned no table");
    const std::string path = std::string(dir) + "/data.json";
    Fd fd;
    fd.fd = ::open(path.c_str(), O_RDONLY);
    if (fd.fd < 0) return prep_fail(M6A_EIO, "cannot open %s", path.c_str());
    struct stat stt;
    if (fstat(fd.fd, &stt) != 0) return prep_fail(M6A_EIO, "cannot stat %s", path.c_str());
    const int64_t n = (int64_t)stt.st_size, S = T->n_sites, R = T->n_reads;
    if (S == 0) return prep_fail(M6A_EFORMAT, "no site with at least %d reads", min_reads);
    if (S > 0x7fffffffll) return prep_fail(M6A_EINVAL, "more than 2^31 sites");
    P.off.assign((size_t)S + 1, 0);
    for (int64_t i = 0; i < S; i++) P.off[(size_t)i + 1] = P.off[(size_t)i] + T->site_reads[i];
    P.tx.assign(T->site_tx, T->site_tx + S);
    P.pos.assign(T->pos, T->pos + S);
    P.k7.assign((size_t)S * 7, 0);
    P.tx_off.assign(T->tx_off, T->tx_off + T->n_tx + 1);
    P.blob.assign(T->tx_blob, (size_t)T->tx_off[T->n_tx]);
    std::vector<JsonSite> hs((size_t)S);
    std::vector<uint8_t> take((size_t)S, 0), status((size_t)S, 0);          // take: the range is inside the file
    std::vector<uint32_t> order;                                             // those sites by their first byte: the upload meets them so
    for (int64_t i = 0; i < S; i++) {
        const int64_t a = T->start[i], b = T->end[i];
        const bool ok = a >= 0 && b <= n && a < b && b - a < 0x7fffffffll;
        hs[(size_t)i] = JsonSite{ok ? a : 0, ok ? b : 0, T->pos[i], T->site_tx[i], 0};
        if (ok) order.push_back((uint32_t)i);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hs[a].start < hs[b].start; });
    double host_ms = now_ms() - t1;

    // ---- device memory: the file, the table and everything the handle keeps, all under the budget before a byte goes up
    DevMem m;
    if ((rc = open_device(device_id, m, "run `inference --loader host` (the default), which streams X from host memory"))) return rc;
    const int64_t nb = std::max<int64_t>(1, (n + kScanBytes - 1) / kScanBytes);
    std::vector<uint64_t> nk, voc = vocab_keys();
    std::vector<int32_t> nix;
    norm_keys(norm_kmers, n_norm, nk, nix);
    uint8_t *df, *dblob, *site_kmers, *site_k7, *dstatus;
    JsonSite *dsites;
    int64_t *doff, *dtx_off, *site_pos;
    int32_t *row_start, *site_norm, *dnix;
    uint32_t *site_tx;
    uint64_t *dnk, *dvoc;
    double *dmean, *dstd, *dids, *mr;
    float *X, *rp, *sp;
    if ((rc = m.alloc(df, (size_t)(nb * kScanBytes), "data.json")) || (rc = m.alloc(dsites, (size_t)S, "the site table")) ||
        (rc = m.alloc(doff, (size_t)S + 1, "the offsets")) || (rc = m.alloc(dblob, P.blob.size() + 1, "transcript names")) ||
        (rc = m.alloc(dtx_off, P.tx_off.size(), "transcript names")) || (rc = m.alloc(row_start, (size_t)R + 1, "row starts")) ||
        (rc = m.alloc(site_norm, (size_t)S * 3, "sites")) || (rc = m.alloc(site_kmers, (size_t)S * 3, "site k-mers")) ||
        (rc = m.alloc(site_k7, (size_t)S * 7, "sites")) || (rc = m.alloc(dstatus, (size_t)S, "the status bytes")) ||
        (rc = m.alloc(site_tx, (size_t)S, "sites")) || (rc = m.alloc(site_pos, (size_t)S, "sites")) ||
        (rc = m.alloc(dnk, nk.size() + 1, "norm")) || (rc = m.alloc(dnix, nix.size() + 1, "norm")) || (rc = m.alloc(dvoc, voc.size(), "norm")) ||
        (rc = m.alloc(dmean, (size_t)n_norm * 3 + 1, "norm")) || (rc = m.alloc(dstd, (size_t)n_norm * 3 + 1, "norm")) ||
        (rc = m.alloc(X, (size_t)R * 9, "X")) || (rc = m.alloc(dids, (size_t)R + 1, "read ids")) ||
        (rc = m.alloc(rp, (size_t)R, "read probabilities")) || (rc = m.alloc(sp, (size_t)S, "site probabilities")) ||
        (rc = m.alloc(mr, (size_t)S, "mod ratios")))
        return rc;

    // ---- upload: data.json whole through the pinned pair; the table goes up beside it
    Streams St;
    int64_t chunk = 0;
    if ((rc = St.open(nb * kScanBytes, chunk))) return rc;
    hipStream_t s = St.s[0];
    const double t_up = now_ms();
    if ((rc = h2d(dsites, hs.data(), (size_t)S, s)) || (rc = h2d(doff, P.off.data(), (size_t)S + 1, s)) ||
        (rc = h2d(dblob, (const uint8_t *)P.blob.data(), P.blob.size(), s)) || (rc = h2d(dtx_off, P.tx_off.data(), P.tx_off.size(), s)) ||
        (rc = h2d(site_tx, P.tx.data(), (size_t)S, s)) || (rc = h2d(site_pos, P.pos.data(), (size_t)S, s)) ||
        (rc = h2d(dnk, nk.data(), nk.size(), s)) || (rc = h2d(dnix, nix.data(), nix.size(), s)) || (rc = h2d(dvoc, voc.data(), voc.size(), s)) ||
        (rc = h2d(dmean, norm_mean, (size_t)n_norm * 3, s)) || (rc = h2d(dstd, norm_std, (size_t)n_norm * 3, s)))
        return rc;
    // The host needs each site's 7-mer for the CSV rows and only a status byte comes back per site: it walks the header of every site
    // in the pinned chunk that holds its first byte, under that chunk's copy, with the core the kernels compile.
    size_t nxt = 0;
    std::vector<uint8_t> edge;
    rc = upload_range(device_id, fd.fd, path.c_str(), St, df, 0, n, chunk, [&](int slot, int64_t at, int64_t len) -> int {
        const uint8_t *const pin = (const uint8_t *)St.pin[slot];
        for (; nxt < order.size() && hs[order[nxt]].start < at + len; nxt++) {
            const uint32_t i = order[nxt];
            const JsonSite &h = hs[i];
            const uint8_t *tx = (const uint8_t *)P.blob.data() + P.tx_off[h.tx], *body;
            const int64_t tx_len = P.tx_off[h.tx + 1] - P.tx_off[h.tx];
            uint64_t k7 = 0;
            int r = header(pin + (h.start - at), pin + (std::min(h.end, at + len) - at), tx, tx_len, h.pos, &k7, &body);
            if (r && h.end > at + len) {                    // the header may straddle the chunk's end: its bytes from the file
                edge.resize((size_t)std::min<int64_t>(h.end - h.start, tx_len + 4096));
                const int rc2 = read_fully(fd.fd, edge.data(), (int64_t)edge.size(), h.start, path.c_str());
                if (rc2) return rc2;
                r = header(edge.data(), edge.data() + edge.size(), tx, tx_len, h.pos, &k7, &body);
            }
            if (!r) {
                for (int j = 0; j < 7; j++) P.k7[(size_t)i * 7 + j] = (char)(k7 >> (8 * (6 - j)));
                take[i] = 1;
            }
        }
        return M6A_OK;
    });
    if (rc) return rc;
    PCHK(hipStreamSynchronize(s));
    ms[0] = now_ms() - t_up;
    ms[6] = ms[0] > 0 ? (double)n / (ms[0] * 1e6) : 0;

    // ---- the kernels; a status byte per site comes back
    t1 = now_ms();
    const unsigned blocks = (unsigned)((S + kJsonWaves - 1) / kJsonWaves);
    json_scan_kernel<<<blocks, kBlk, 0, s>>>(df, dsites, doff, S, dblob, dtx_off, dnk, dnix, (int)nk.size(), dvoc, (int)voc.size(), row_start, site_norm,
                                             site_kmers, site_k7, dstatus);
    PCHK(hipGetLastError());
    json_rows_kernel<<<blocks, kBlk, 0, s>>>(df, dsites, doff, S, row_start, site_norm, dmean, dstd, n_norm, X, dids, dstatus);
    PCHK(hipGetLastError());
    if ((rc = d2h(status.data(), dstatus, (size_t)S, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    ms[3] = now_ms() - t1;

    // ---- declined sites, in ascending order through the loader's own per-site body: their rows, or its first error
    t1 = now_ms();
    std::vector<int64_t> decl;
    for (int64_t i = 0; i < S; i++)
        if (status[(size_t)i] || !take[(size_t)i]) decl.push_back(i);
    if (!decl.empty()) {
        int64_t rows = 0;
        for (int64_t i : decl) rows += T->site_reads[i];
        std::vector<float> hX((size_t)rows * 9);
        std::vector<double> hid((size_t)rows);
        std::vector<uint8_t> hk((size_t)decl.size() * 3);
        std::vector<char> h7((size_t)decl.size() * 7);
        hrc = host->rows(info.p, decl.data(), (int64_t)decl.size(), norm_kmers, norm_mean, norm_std, n_norm, n_threads, hX.data(), hid.data(), hk.data(),
                         h7.data());
        if (hrc) return json_host_fail(host, hrc);
        int64_t at = 0;
        for (size_t k = 0; k < decl.size(); k++) {
            const int64_t i = decl[k], r0 = P.off[(size_t)i], nr = T->site_reads[i];
            if ((rc = h2d(X + 9 * r0, hX.data() + 9 * at, (size_t)nr * 9, s)) || (rc = h2d(dids + r0, hid.data() + at, (size_t)nr, s)) ||
                (rc = h2d(site_kmers + 3 * i, hk.data() + 3 * k, 3, s)) || (rc = h2d(site_k7 + 7 * i, (const uint8_t *)h7.data() + 7 * k, 7, s)))
                return rc;
            memcpy(&P.k7[(size_t)i * 7], h7.data() + 7 * k, 7);
            at += nr;
        }
        PCHK(hipStreamSynchronize(s));
    }
    ms[4] = host_ms + (now_ms() - t1);

    // ---- the read ids: all that comes back per read
    t1 = now_ms();
    P.ids.resize((size_t)R);
    if ((rc = d2h(P.ids.data(), dids, (size_t)R, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    ms[5] = now_ms() - t1;

    for (const void *p : {(const void *)X, (const void *)site_kmers, (const void *)doff, (const void *)rp, (const void *)sp, (const void *)mr,
                          (const void *)site_tx, (const void *)site_pos, (const void *)site_k7, (const void *)dids}) {
        P.held += m.size_of(p);
        m.detach(p);
        P.dev.push_back((void *)p);
    }
    P.csv_tx = site_tx; P.csv_pos = site_pos; P.csv_k7 = site_k7; P.csv_ids = dids;
    m6a_prep_sites_info &I = P.info;
    I.n_sites = S; I.n_reads = R; I.n_tx = T->n_tx;
    I.X = X; I.site_kmers = site_kmers; I.off = doff; I.read_prob = rp; I.site_prob = sp; I.mod_ratio = mr;
    I.off_host = P.off.data(); I.site_tx = P.tx.data(); I.site_pos = P.pos.data(); I.site_kmer7 = P.k7.data();
    I.tx_blob = P.blob.data(); I.tx_off = P.tx_off.data(); I.read_ids = P.ids.data();
    P.rep.assign((size_t)R, 0);
    I.n_rep = 1; I.read_rep = P.rep.data();
    I.n_windows = 1; I.window_bytes = 0;
    I.n_declined_sites = (int64_t)decl.size();
    I.d2h_bytes = g_d2h;
    I.peak_bytes = (int64_t)m.peak;
    ms[7] = now_ms() - t_all;
    return M6A_OK;
}

}  // namespace

extern "C" int m6a_json_sites_build(int device_id, const char *const *dirs, int n_dirs, int min_reads, const char *norm_kmers,
                                    const double *norm_mean, const double *norm_std, int n_norm, const m6a_json_host_half *host, int n_threads,
                                    m6a_prep_sites **out)
{
    if (!dirs || !out || n_dirs < 1 || !dirs[0]) return prep_fail(M6A_EINVAL, "null argument");
    *out = nullptr;
    // refused before anything is opened or allocated
    if (n_dirs > 1)
        return prep_fail(M6A_EINVAL, "the device loader takes one input directory, not %d: replicates are pooled by the host loader "
                         "(`inference --loader host`)", n_dirs);
    const size_t dl = strlen(dirs[0]);
    if (dl >= 9 && strcmp(dirs[0] + dl - 9, ".m6astore") == 0)
        return prep_fail(M6A_EINVAL, "%s is a binary site store, which holds no JSON to parse: `inference --loader host` maps it", dirs[0]);
    if (!host || !host->open || !host->table || !host->rows || !host->free) return prep_fail(M6A_EINVAL, "the host half is missing");
    if (n_norm < 0 || (n_norm > 0 && (!norm_kmers || !norm_mean || !norm_std))) return prep_fail(M6A_EINVAL, "bad normalisation arguments");
    m6a_prep_sites *p = new (std::nothrow) m6a_prep_sites;
    if (!p) return prep_fail(M6A_ENOMEM, "out of host memory");
    p->device = device_id;
    const int rc = guarded([&] { return json_impl(device_id, dirs[0], min_reads, norm_kmers, norm_mean, norm_std, n_norm, host, n_threads, *p); });
    if (rc) { delete p; return rc; }
    *out = p;
    return M6A_OK;
}
#endif  // M6A_JSON_DEVICE_PART
