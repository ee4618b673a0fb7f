// m6a_deflate.h -- the BGZF writer of `eventalign_inference --compress` (include/m6a.h states it): text in, BGZF blocks out.
//
// Part 1, the deflate core: plain C++ marked for host and device, no HIP in it.  m6a_io.cpp compiles it for the CPU
// (m6a_io_bgzf_deflate and m6a_io_bgzf_deflate_level, and two programs of tests/ under the sanitizers); m6a_prep.hip compiles the same text for gfx950, and
// both give the same bytes: nothing below depends on timing or on the order in which lanes run.
//   block       at most kBlockInput = 65 280 bytes of text become one BGZF block: the 18-byte header, one raw DEFLATE stream
//               (RFC 1951), CRC-32 and ISIZE.  At level 1 the stream is ONE block of fixed Huffman codes (BTYPE 01), or one stored block
//               (BTYPE 00) when the coded stream would not be smaller than 5 + n bytes -- so a BGZF block is at most
//               18 + 5 + 65 280 + 8 bytes, under the format's 65 536.
//   parts       the text of a block is cut into 64 parts of per = ceil(n / 64) bytes (the last may be shorter, parts may be empty);
//               a lane (the CPU: a loop index) parses its part greedily and on its own.  Matches are 3..258 bytes long, start and
//               end inside the part, and reach back at most kReach = 256 bytes in front of the part -- into earlier parts, never in
//               front of the block's first byte; every distance is far below 32 768.
//   finder      a table of kSets x kWays 16-bit positions per lane (512 bytes; 32 KB of LDS for a wave), indexed by a hash of the
//               next three bytes; a set keeps the last kWays positions with that hash, newest first, and the longest match among
//               them wins, the nearer one at equal length.  The table is primed with the kReach positions in front of the part.
//               Only its own lane reads or writes a lane's table.
//   merging     a part's bit string (part 0 starts with the three header bits, part 63 ends with the end-of-block code) is formed
//               twice: part_bits() gives its length and its first byte; after an exclusive sum of the lengths part_emit() forms it
//               again and stores it at its bit offset.  A byte of the stream is stored by the lane whose string holds the byte's
//               first bit; the bits of later parts that share the byte come from their first bytes.  So every byte has one
//               writer, and no byte is read back.
//   CRC-32      m6a_bgzf::crc_lane, the 64 terms XORed.
//   level 2     the same blocks, parts, finder and tokens (part_walk is the one walk of both levels); only how tokens become bits
//               changes.  The walk that measures the fixed strings also counts the block's literal/length symbols and distance codes
//               (Hist); block_plan builds from the counts the two length-limited codes (code_lengths: Moffat and Katajainen's in-place
//               depths, cut to 15 bits with the Kraft repair of zlib and miniz; canonical), the run-coded header with its 7-bit code,
//               and chooses by bits: dynamic where it is smaller than fixed, header included; stored where the winner would take
//               5 + n bytes or more.  A dynamic block is measured and emitted a second time under its codes (part_bits_dyn,
//               part_emit_dyn); its header is a 65th bit string in front of part 0 (header_emit).  Everything is integer arithmetic on
//               counts, so neither the order in which parts are counted nor who counts them can change a byte.
//
// Part 2 (M6A_DEFLATE_DEVICE_PART, m6a_prep.hip only): the kernels, m6a_bgzf_deflate and m6a_prep_sites_write_csv_bgzf.
//   layout      one wave per BGZF block, one wave per workgroup: the 64 tables (32 KB), the CRC byte table (1 KB) and the parts'
//               lengths and first bytes (0.5 KB) in LDS, so four waves share a CU's 160 KB.  The text is read from global memory.
//   placement   block sizes are known only after the parse: bgzf_deflate_kernel writes block b into slot b of 64 KiB and its size
//               into size[b]; an exclusive scan gives the offsets and bgzf_pack_kernel moves every block to its place in the packed
//               buffer.  All stores are vector stores in plain C++.
//   status      the packed sizes and the count of stored blocks come back in one record of three words per round.
//   level 2     bgzf_deflate_dyn_kernel, beside bgzf_deflate_kernel, which stays as it was with its 34 KB and its launch.  Of the two
//               layouts for the counts -- a 16-bit histogram per lane (316 x 64 x 2 B = 40 KB: 75 KB a wave, two waves a CU, lengths by
//               a dot product, two walks) or one histogram of the wave through LDS integer atomics (316 words; a third walk for a
//               block that comes out dynamic) -- this is the second: the kernel has 38.6 KB of LDS, so four waves still share a CU,
//               which a kernel whose lanes wait on byte loads needs more than it needs to save a walk; fixed and stored blocks pay
//               no third walk; and the atomics add integers, so the counts are exact whatever the order.  Neither layout has been
//               timed.  Lane 0 runs block_plan (at most 286 symbols: an insertion sort and three passes) while the other lanes wait
//               at a barrier; the codes, the header and the scratch are in LDS.  The record has a fourth word, the dynamic blocks.
#ifndef M6A_DEFLATE_H
#define M6A_DEFLATE_H
#include <stdint.h>

#include "m6a_bgzf.h"

namespace m6a_deflate {

constexpr int32_t kBlockInput = 0xff00;       // text bytes per BGZF block, as htslib's bgzip and m6anet_amd/bgzf.py cut them
constexpr int32_t kSlot = 65536;              // the largest BGZF block
constexpr int kParts = 64;
constexpr int32_t kReach = 256;               // bytes in front of a part that its matches may start in
constexpr int kSets = 128, kWays = 2;
constexpr int kTableEntries = kSets * kWays * kParts;      // uint16_t: 32 KB
constexpr uint16_t kNone = 0xffff;            // positions are below 65 280
constexpr int32_t kHeader = 18, kFooter = 8;
constexpr int32_t kEofBytes = 28;

M6A_HD inline int64_t n_blocks(int64_t n) { return (n + kBlockInput - 1) / kBlockInput; }
M6A_HD inline int64_t bound(int64_t n) { return n_blocks(n) * kSlot + kEofBytes; }

M6A_HD inline uint8_t eof_byte(int i)         // the specification's 28-byte end-of-file marker
{
    const uint8_t m[kEofBytes] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return m[i];
}

// ---- the bit strings ----
M6A_HD inline uint32_t rev(uint32_t v, int n)               // the low n <= 16 bits of v, reversed
{
    v = (v & 0x5555u) << 1 | (v >> 1 & 0x5555u);
    v = (v & 0x3333u) << 2 | (v >> 2 & 0x3333u);
    v = (v & 0x0f0fu) << 4 | (v >> 4 & 0x0f0fu);
    v = (v & 0x00ffu) << 8 | (v >> 8 & 0x00ffu);
    return v >> (16 - n);
}

struct Count {                                // a part's length in bits and its first byte
    uint32_t bits = 0, head = 0;
    M6A_HD void put(uint32_t v, int n)        // n <= 32 - 7
    {
        if (bits < 8) head |= (v << bits) & 0xff;
        bits += (uint32_t)n;
    }
};

struct Emit {                                 // a part's bit string stored from bit `at` of out on; the bits below the first byte
    uint8_t *out;                             // boundary are dropped (the lane in front stores that byte)
    uint32_t skip;                            // bits still to drop
    uint32_t byte;                            // index of the next byte to store
    uint64_t acc = 0;
    int cnt = 0;
    M6A_HD Emit(uint8_t *o, uint32_t at) : out(o), skip((8 - (at & 7)) & 7), byte((at + 7) >> 3) {}
    M6A_HD void put(uint32_t v, int n)
    {
        if (skip) {
            const int k = (int)skip < n ? (int)skip : n;
            v >>= k;
            n -= k;
            skip -= (uint32_t)k;
            if (!n) return;
        }
        acc |= (uint64_t)v << cnt;
        cnt += n;
        while (cnt >= 8) {
            out[byte++] = (uint8_t)acc;
            acc >>= 8;
            cnt -= 8;
        }
    }
};

template <class Sink> M6A_HD inline void put_literal(Sink &s, uint32_t b)
{
    if (b < 144) s.put(rev(0x30 + b, 8), 8);
    else s.put(rev(0x190 + (b - 144), 9), 9);
}

// the length symbol 257..285 of a match of len bytes, 3 <= len <= 258, and its extra bits
M6A_HD inline void length_symbol(int32_t len, uint32_t *sym, uint32_t *ext, uint32_t *extra)
{
    const uint32_t l = (uint32_t)(len - 3);
    *ext = *extra = 0;
    if (l < 8) *sym = 257 + l;
    else if (l == 255) *sym = 285;
    else {
        *ext = (uint32_t)(31 - __builtin_clz(l)) - 2;
        *sym = 261 + 4 * *ext + ((l >> *ext) & 3);
        *extra = l & ((1u << *ext) - 1);
    }
}
// the distance code 0..29 of dist, 1 <= dist <= 32768, and its extra bits
M6A_HD inline void dist_symbol(int32_t dist, uint32_t *code, uint32_t *ext, uint32_t *extra)
{
    const uint32_t d = (uint32_t)(dist - 1);
    *code = d;
    *ext = *extra = 0;
    if (d >= 4) {
        *ext = (uint32_t)(31 - __builtin_clz(d)) - 1;
        *code = 2 * *ext + 2 + ((d >> *ext) & 1);
        *extra = d & ((1u << *ext) - 1);
    }
}

template <class Sink> M6A_HD inline void put_match(Sink &s, int32_t len, int32_t dist)      // 3 <= len <= 258, 1 <= dist <= 32768
{
    const uint32_t l = (uint32_t)(len - 3);
    uint32_t sym, ext = 0, extra = 0;
    if (l < 8) sym = 257 + l;
    else if (l == 255) sym = 285;
    else {
        ext = (uint32_t)(31 - __builtin_clz(l)) - 2;
        sym = 261 + 4 * ext + ((l >> ext) & 3);
        extra = l & ((1u << ext) - 1);
    }
    if (sym < 280) s.put(rev(sym - 256, 7), 7);
    else s.put(rev(0xc0 + (sym - 280), 8), 8);
    if (ext) s.put(extra, (int)ext);
    const uint32_t d = (uint32_t)(dist - 1);
    uint32_t code = d, dext = 0;
    if (d >= 4) {
        dext = (uint32_t)(31 - __builtin_clz(d)) - 1;
        code = 2 * dext + 2 + ((d >> dext) & 1);
    }
    s.put(rev(code, 5), 5);
    if (dext) s.put(d & ((1u << dext) - 1), (int)dext);
}

template <class Sink> struct Fixed {          // tokens as the fixed codes of RFC 1951, 3.2.6
    Sink &s;
    M6A_HD void literal(uint32_t b) { put_literal(s, b); }
    M6A_HD void match(int32_t len, int32_t dist) { put_match(s, len, dist); }
};

// ---- the finder: lane's table is tab[(set * kWays + way) * kParts + lane] ----
M6A_HD inline uint32_t hash3(const uint8_t *p) { return ((uint32_t)(p[0] | p[1] << 8 | p[2] << 16) * 0x9e3779b1u) >> 25; }      // < kSets

M6A_HD inline void insert(uint16_t *tab, int lane, const uint8_t *in, int32_t q)
{
    uint16_t *t = tab + (hash3(in + q) * kWays) * kParts + lane;
    t[kParts] = t[0];
    t[0] = (uint16_t)q;
}

M6A_HD inline void part_range(int32_t n, int lane, int32_t *lo, int32_t *hi)
{
    const int32_t per = (n + kParts - 1) / kParts;
    *lo = lane * per < n ? lane * per : n;
    *hi = *lo + per < n ? *lo + per : n;
}

// the tokens of part `lane` of in[0, n), n <= kBlockInput, to t.literal / t.match: the one walk both levels code
template <class Tok> M6A_HD inline void part_walk(const uint8_t *in, int32_t n, int lane, uint16_t *tab, Tok &t)
{
    int32_t lo, hi;
    part_range(n, lane, &lo, &hi);
    for (int e = 0; e < kSets * kWays; e++) tab[e * kParts + lane] = kNone;
    for (int32_t q = lo > kReach ? lo - kReach : 0; q < lo; q++)
        if (q + 2 < n) insert(tab, lane, in, q);
    for (int32_t i = lo; i < hi;) {
        int32_t best = 0, best_at = 0;
        if (i + 2 < hi) {
            const uint16_t *w0 = tab + (hash3(in + i) * kWays) * kParts + lane;
            const int32_t room = hi - i < 258 ? hi - i : 258;
            for (int w = 0; w < kWays; w++) {
                const int32_t c = w0[w * kParts];
                if (c == kNone) break;
                int32_t l = 0;                              // c < i: the table holds positions already passed
                while (l < room && in[c + l] == in[i + l]) l++;
                if (l > best) { best = l; best_at = c; }
            }
            insert(tab, lane, in, i);
        }
        if (best >= 3 && i - best_at <= 32768) {
            t.match(best, i - best_at);
            for (int32_t q = i + 1; q < i + best; q++)
                if (q + 2 < hi) insert(tab, lane, in, q);
            i += best;
        } else {
            t.literal(in[i]);
            i++;
        }
    }
}

// the bit string of part `lane` under the fixed codes, into the sink
template <class Sink> M6A_HD inline void part_code(const uint8_t *in, int32_t n, int lane, uint16_t *tab, Sink &s)
{
    if (lane == 0) s.put(3, 3);                             // BFINAL = 1, BTYPE = 01
    Fixed<Sink> f{s};
    part_walk(in, n, lane, tab, f);
    if (lane == kParts - 1) s.put(0, 7);                    // end of block
}

M6A_HD inline void part_bits(const uint8_t *in, int32_t n, int lane, uint16_t *tab, uint32_t *bits, uint32_t *head)
{
    Count c;
    part_code(in, n, lane, tab, c);
    *bits = c.bits;
    *head = c.head;
}

// the last byte a string owns, filled up from the parts `next`.. behind it
M6A_HD inline void emit_finish(Emit &e, int next, const uint32_t *bits, const uint32_t *head)
{
    if (e.cnt && !e.skip) {
        for (int q = next; q < kParts && e.cnt < 8; q++) {
            const int k = (int)bits[q] < 8 - e.cnt ? (int)bits[q] : 8 - e.cnt;
            e.acc |= (uint64_t)(head[q] & ((1u << k) - 1)) << e.cnt;
            e.cnt += k;
        }
        e.out[e.byte] = (uint8_t)e.acc;
    }
}

// start = the sum of bits[0, lane); out = the first byte of the deflate stream
M6A_HD inline void part_emit(const uint8_t *in, int32_t n, int lane, uint16_t *tab, uint32_t start, const uint32_t *bits, const uint32_t *head,
                             uint8_t *out)
{
    Emit e(out, start);
    part_code(in, n, lane, tab, e);
    emit_finish(e, lane + 1, bits, head);
}

M6A_HD inline void put_header(uint8_t *blk, int32_t total)
{
    const uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; i++) blk[i] = h[i];
    blk[16] = (uint8_t)(total - 1);
    blk[17] = (uint8_t)((total - 1) >> 8);
}
M6A_HD inline void put_footer(uint8_t *p, uint32_t crc, int32_t n)
{
    for (int i = 0; i < 4; i++) {
        p[i] = (uint8_t)(crc >> (8 * i));
        p[4 + i] = (uint8_t)((uint32_t)n >> (8 * i));
    }
}
// bytes of the coded stream of `bits` bits, or of the stored block when that is not larger
M6A_HD inline int32_t stream_bytes(uint32_t bits, int32_t n, bool *stored)
{
    const int32_t coded = (int32_t)((bits + 7) >> 3);
    *stored = coded >= 5 + n;
    return *stored ? 5 + n : coded;
}
M6A_HD inline void put_stored_head(uint8_t *p, int32_t n)
{
    p[0] = 1;
    p[1] = (uint8_t)n;
    p[2] = (uint8_t)(n >> 8);
    p[3] = (uint8_t)~n;
    p[4] = (uint8_t)(~n >> 8);
}

// ---- level 2: the block's own Huffman codes (BTYPE 10) over the same tokens ----
constexpr int kLitLen = 286, kDist = 30, kCodeLen = 19;     // the three alphabets
constexpr int kSymbols = kLitLen + kDist;                   // a block's counts: literal/length symbols, then distance codes
constexpr int kMaxBits = 15, kCodeLenBits = 7;
constexpr int kWork = 2 * kLitLen;                          // words of scratch for code_lengths

struct PlainAdd {                             // how a count grows where one thread holds the histogram (the device part adds LDS atomics)
    M6A_HD static void add(uint32_t *p) { ++*p; }
};

// A part's tokens counted into the block's histogram; beside it the part's string under the fixed codes (level 1's own, by the same
// calls) and the extra bits of its matches, which cost the same under any code.
template <class Add> struct Hist {
    uint32_t *freq;
    Count fixed;
    uint32_t extra;
    M6A_HD void literal(uint32_t b)
    {
        Add::add(freq + b);
        put_literal(fixed, b);
    }
    M6A_HD void match(int32_t len, int32_t dist)
    {
        uint32_t sym, ext, x, code, dext;
        length_symbol(len, &sym, &ext, &x);
        dist_symbol(dist, &code, &dext, &x);
        Add::add(freq + sym);
        Add::add(freq + kLitLen + code);
        extra += ext + dext;
        put_match(fixed, len, dist);
    }
};

template <class Add>
M6A_HD inline void part_hist(const uint8_t *in, int32_t n, int lane, uint16_t *tab, uint32_t *freq, uint32_t *bits, uint32_t *head, uint32_t *extra)
{
    Hist<Add> h{freq, Count(), 0};
    if (lane == 0) h.fixed.put(3, 3);
    part_walk(in, n, lane, tab, h);
    if (lane == kParts - 1) {
        h.fixed.put(0, 7);
        Add::add(freq + 256);                               // end of block counts once
    }
    *bits = h.fixed.bits;
    *head = h.fixed.head;
    *extra = h.extra;
}

// Code lengths of at most `limit` bits for freq[0, n_symbols) into out; a symbol of count 0 gets length 0.  The rule: the used symbols
// are sorted by (count, symbol); Moffat and Katajainen's in-place pass gives every one its depth in a minimum-redundancy (Huffman)
// tree; depths over the limit are cut to it and the Kraft sum is repaired as zlib and miniz do -- while it is over 1, a code of the
// limit's length is dropped and one of the longest shorter codes becomes two codes a bit longer; the lengths are then dealt longest
// first to the rarest symbols.  So the code is complete, costs what Huffman's costs wherever that fits the limit, and depends on the
// counts alone.  One used symbol gets length 1 and none gets nothing (RFC 1951, 3.2.7).  limit <= 15, 2^limit >= n_symbols, the
// counts' sum below 2^32; work: 2 * n_symbols words.
M6A_HD inline void code_lengths(const uint32_t *freq, int n_symbols, int limit, uint8_t *out, uint32_t *work)
{
    uint32_t *a = work, *key = work + n_symbols;            // key: the used symbols, then sorted
    int m = 0;
    for (int s = 0; s < n_symbols; s++) {
        out[s] = 0;
        if (freq[s]) key[m++] = (uint32_t)s;
    }
    if (m == 0) return;
    if (m == 1) {
        out[key[0]] = 1;
        return;
    }
    for (int i = 1; i < m; i++) {                           // by count, ascending; equal counts stay in symbol order
        const uint32_t k = key[i];
        int j = i;
        for (; j > 0 && freq[key[j - 1]] > freq[k]; j--) key[j] = key[j - 1];
        key[j] = k;
    }
    for (int i = 0; i < m; i++) a[i] = freq[key[i]];
    a[0] += a[1];                                           // weights of the inner nodes, then parent indices
    int root = 0, leaf = 2;
    for (int next = 1; next < m - 1; next++) {
        if (leaf >= m || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = (uint32_t)next; }
        else a[next] = a[leaf++];
        if (leaf >= m || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = (uint32_t)next; }
        else a[next] += a[leaf++];
    }
    a[m - 2] = 0;                                           // depths of the inner nodes
    for (int next = m - 3; next >= 0; next--) a[next] = a[a[next]] + 1;
    int avail = 1, used = 0, depth = 0, next = m - 1;       // depths of the leaves, the most frequent first
    root = m - 2;
    while (avail > 0) {
        while (root >= 0 && (int)a[root] == depth) { used++; root--; }
        while (avail > used) { a[next--] = (uint32_t)depth; avail--; }
        avail = 2 * used;
        depth++;
        used = 0;
    }
    uint32_t count[kMaxBits + 1];
    for (int l = 0; l <= limit; l++) count[l] = 0;
    for (int i = 0; i < m; i++) count[(int)a[i] < limit ? (int)a[i] : limit]++;
    uint32_t total = 0;
    for (int l = 1; l <= limit; l++) total += count[l] << (limit - l);
    while (total != 1u << limit) {                          // over 1: cutting depths only adds to the sum
        count[limit]--;
        for (int l = limit - 1; l > 0; l--)
            if (count[l]) {
                count[l]--;
                count[l + 1] += 2;
                break;
            }
        total--;
    }
    int at = 0;
    for (int l = limit; l > 0; l--)
        for (uint32_t c = 0; c < count[l]; c++) out[key[at++]] = (uint8_t)l;
}

// the canonical code of len[0, n), every code word reversed as the stream takes it
M6A_HD inline void canonical(const uint8_t *len, int n, uint16_t *code)
{
    uint32_t next[kMaxBits + 2], count[kMaxBits + 1];
    for (int l = 0; l <= kMaxBits; l++) count[l] = 0;
    for (int s = 0; s < n; s++) count[len[s]]++;
    next[1] = 0;
    for (int l = 1; l <= kMaxBits; l++) next[l + 1] = (next[l] + count[l]) << 1;
    for (int s = 0; s < n; s++) code[s] = len[s] ? (uint16_t)rev(next[len[s]]++, len[s]) : (uint16_t)0;
}

struct Codes {                                // a block's two codes
    uint8_t ll_len[kLitLen], d_len[kDist];
    uint16_t ll_code[kLitLen], d_code[kDist];
};

template <class Sink> struct Dynamic {        // tokens as the block's own codes
    Sink &s;
    const Codes &c;
    M6A_HD void literal(uint32_t b) { s.put(c.ll_code[b], c.ll_len[b]); }
    M6A_HD void match(int32_t len, int32_t dist)
    {
        uint32_t sym, ext, extra, code, dext, dextra;
        length_symbol(len, &sym, &ext, &extra);
        s.put(c.ll_code[sym], c.ll_len[sym]);
        if (ext) s.put(extra, (int)ext);
        dist_symbol(dist, &code, &dext, &dextra);
        s.put(c.d_code[code], c.d_len[code]);
        if (dext) s.put(dextra, (int)dext);
    }
};

// part `lane` under the block's codes: no header bits in it (the header is a string of its own in front of part 0)
template <class Sink> M6A_HD inline void part_code_dyn(const uint8_t *in, int32_t n, int lane, uint16_t *tab, const Codes &c, Sink &s)
{
    Dynamic<Sink> d{s, c};
    part_walk(in, n, lane, tab, d);
    if (lane == kParts - 1) s.put(c.ll_code[256], c.ll_len[256]);
}
M6A_HD inline void part_bits_dyn(const uint8_t *in, int32_t n, int lane, uint16_t *tab, const Codes &c, uint32_t *bits, uint32_t *head)
{
    Count k;
    part_code_dyn(in, n, lane, tab, c, k);
    *bits = k.bits;
    *head = k.head;
}
M6A_HD inline void part_emit_dyn(const uint8_t *in, int32_t n, int lane, uint16_t *tab, const Codes &c, uint32_t start, const uint32_t *bits,
                                 const uint32_t *head, uint8_t *out)
{
    Emit e(out, start);
    part_code_dyn(in, n, lane, tab, c, e);
    emit_finish(e, lane + 1, bits, head);
}

// The header of a dynamic block: HLIT, HDIST and HCLEN, the code-length code (limited to 7 bits, built by code_lengths too) and the
// HLIT + HDIST lengths as one sequence of its symbols: a length as itself; a run of r more of the same length as 16s of 3..6 while
// r >= 3; a run of zeros as 18s of 11..138 while 11 or more are left, then one 17 of 3..10, then single zeros.  Trailing unused symbols
// above 256 are not sent; without a match HDIST is one distance code of length 0.
struct Header {
    uint32_t hlit, hdist, hclen, n_rle;
    uint8_t cl_len[kCodeLen];
    uint16_t cl_code[kCodeLen];
    uint8_t rle[kSymbols], rle_extra[kSymbols];
};
M6A_HD inline int cl_order(int i)
{
    const uint8_t o[kCodeLen] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[i];
}
M6A_HD inline void header_build(const Codes &c, Header &h, uint32_t *work)
{
    h.hlit = kLitLen;
    while (h.hlit > 257 && !c.ll_len[h.hlit - 1]) h.hlit--;
    h.hdist = kDist;
    while (h.hdist > 1 && !c.d_len[h.hdist - 1]) h.hdist--;
    const uint32_t total = h.hlit + h.hdist;
    uint32_t *freq = work;                                  // 19 counts; code_lengths' scratch behind them
    for (int s = 0; s < kCodeLen; s++) freq[s] = 0;
    h.n_rle = 0;
    auto len_at = [&](uint32_t i) -> uint32_t { return i < h.hlit ? c.ll_len[i] : c.d_len[i - h.hlit]; };
    auto put = [&](uint32_t sym, uint32_t extra) {
        h.rle[h.n_rle] = (uint8_t)sym;
        h.rle_extra[h.n_rle++] = (uint8_t)extra;
        freq[sym]++;
    };
    for (uint32_t i = 0; i < total;) {
        const uint32_t v = len_at(i);
        uint32_t run = 1;
        while (i + run < total && len_at(i + run) == v) run++;
        i += run;
        if (v == 0) {
            while (run >= 11) { const uint32_t k = run < 138 ? run : 138; put(18, k - 11); run -= k; }
            if (run >= 3) { put(17, run - 3); run = 0; }
            while (run--) put(0, 0);
        } else {
            put(v, 0);
            run--;
            while (run >= 3) { const uint32_t k = run < 6 ? run : 6; put(16, k - 3); run -= k; }
            while (run--) put(v, 0);
        }
    }
    code_lengths(freq, kCodeLen, kCodeLenBits, h.cl_len, work + 32);
    canonical(h.cl_len, kCodeLen, h.cl_code);
    h.hclen = kCodeLen;
    while (h.hclen > 4 && !h.cl_len[cl_order((int)h.hclen - 1)]) h.hclen--;
}
template <class Sink> M6A_HD inline void header_put(Sink &s, const Header &h)
{
    s.put(5, 3);                                            // BFINAL = 1, BTYPE = 10
    s.put(h.hlit - 257, 5);
    s.put(h.hdist - 1, 5);
    s.put(h.hclen - 4, 4);
    for (uint32_t i = 0; i < h.hclen; i++) s.put(h.cl_len[cl_order((int)i)], 3);
    for (uint32_t i = 0; i < h.n_rle; i++) {
        const uint32_t sym = h.rle[i];
        s.put(h.cl_code[sym], h.cl_len[sym]);
        if (sym >= 16) s.put(h.rle_extra[i], sym == 16 ? 2 : sym == 17 ? 3 : 7);
    }
}
// the header from bit 0 of out on; its last byte is filled up from the parts
M6A_HD inline void header_emit(const Header &h, const uint32_t *bits, const uint32_t *head, uint8_t *out)
{
    Emit e(out, 0);
    header_put(e, h);
    emit_finish(e, 0, bits, head);
}

// The choice, from the block's counts (freq), the extra bits of its matches and its length under the fixed codes: builds both codes
// and the header, and returns the BTYPE -- 2 when the dynamic stream, header included, has fewer bits than the fixed one, else 1, and
// 0 when the winner would not be smaller than the stored block.  *hdr_bits: the header's length.  One thread runs this.
M6A_HD inline int block_plan(const uint32_t *freq, uint32_t extra, uint32_t fixed_bits, int32_t n, Codes &c, Header &h, uint32_t *work, uint32_t *hdr_bits)
{
    code_lengths(freq, kLitLen, kMaxBits, c.ll_len, work);
    code_lengths(freq + kLitLen, kDist, kMaxBits, c.d_len, work);
    canonical(c.ll_len, kLitLen, c.ll_code);
    canonical(c.d_len, kDist, c.d_code);
    header_build(c, h, work);
    Count k;
    header_put(k, h);
    *hdr_bits = k.bits;
    uint32_t dyn = k.bits + extra;
    for (int s = 0; s < kLitLen; s++) dyn += freq[s] * c.ll_len[s];
    for (int s = 0; s < kDist; s++) dyn += freq[kLitLen + s] * c.d_len[s];
    bool stored;
    (void)stream_bytes(dyn < fixed_bits ? dyn : fixed_bits, n, &stored);
    return stored ? 0 : dyn < fixed_bits ? 2 : 1;
}

// One block on the CPU: in[0, n), 0 < n <= kBlockInput, to blk (kSlot bytes of room); returns its size.  tab: kTableEntries entries.
inline int32_t block_host(const uint8_t *in, int32_t n, uint8_t *blk, uint16_t *tab, const uint32_t *crc_tab, bool *stored)
{
    uint32_t bits[kParts], head[kParts], start[kParts], sum = 0, crc = 0;
    for (int lane = 0; lane < kParts; lane++) part_bits(in, n, lane, tab, &bits[lane], &head[lane]);
    for (int lane = 0; lane < kParts; lane++) { start[lane] = sum; sum += bits[lane]; }
    const int32_t body = stream_bytes(sum, n, stored), total = kHeader + body + kFooter;
    put_header(blk, total);
    if (*stored) {
        put_stored_head(blk + kHeader, n);
        for (int32_t i = 0; i < n; i++) blk[kHeader + 5 + i] = in[i];
    } else
        for (int lane = 0; lane < kParts; lane++) part_emit(in, n, lane, tab, start[lane], bits, head, blk + kHeader);
    for (int lane = 0; lane < kParts; lane++) crc ^= m6a_bgzf::crc_lane(crc_tab, in, n, lane);
    put_footer(blk + kHeader + body, crc, n);
    return total;
}

// text[0, n) as BGZF blocks into out (bound(n) bytes of room), without the end-of-file marker; returns the bytes written
inline int64_t blocks_host(const uint8_t *text, int64_t n, uint8_t *out, int64_t *n_stored)
{
    uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; i++) crc_tab[i] = m6a_bgzf::crc_entry(i);
    uint16_t *tab = new uint16_t[kTableEntries];
    int64_t at = 0;
    for (int64_t off = 0; off < n; off += kBlockInput) {
        bool stored;
        at += block_host(text + off, (int32_t)(n - off < kBlockInput ? n - off : kBlockInput), out + at, tab, crc_tab, &stored);
        if (stored && n_stored) ++*n_stored;
    }
    delete[] tab;
    return at;
}

// One block on the CPU at level 1 or 2; *btype: the deflate block type it came out as
inline int32_t block_host(const uint8_t *in, int32_t n, uint8_t *blk, uint16_t *tab, const uint32_t *crc_tab, int level, int *btype)
{
    if (level != 2) {
        bool stored;
        const int32_t total = block_host(in, n, blk, tab, crc_tab, &stored);
        *btype = stored ? 0 : 1;
        return total;
    }
    uint32_t freq[kSymbols] = {0}, work[kWork], bits[kParts], head[kParts], start[kParts], extra = 0, sum = 0, hdr_bits = 0, crc = 0;
    for (int lane = 0; lane < kParts; lane++) {
        uint32_t x;
        part_hist<PlainAdd>(in, n, lane, tab, freq, &bits[lane], &head[lane], &x);
        extra += x;
        sum += bits[lane];
    }
    Codes c;
    Header h;
    *btype = block_plan(freq, extra, sum, n, c, h, work, &hdr_bits);
    if (*btype == 2) {
        for (int lane = 0; lane < kParts; lane++) part_bits_dyn(in, n, lane, tab, c, &bits[lane], &head[lane]);
        sum = hdr_bits;
    } else
        sum = 0;
    for (int lane = 0; lane < kParts; lane++) { start[lane] = sum; sum += bits[lane]; }
    const int32_t body = *btype == 0 ? 5 + n : (int32_t)((sum + 7) >> 3), total = kHeader + body + kFooter;
    put_header(blk, total);
    if (*btype == 0) {
        put_stored_head(blk + kHeader, n);
        for (int32_t i = 0; i < n; i++) blk[kHeader + 5 + i] = in[i];
    } else if (*btype == 1)
        for (int lane = 0; lane < kParts; lane++) part_emit(in, n, lane, tab, start[lane], bits, head, blk + kHeader);
    else {
        header_emit(h, bits, head, blk + kHeader);
        for (int lane = 0; lane < kParts; lane++) part_emit_dyn(in, n, lane, tab, c, start[lane], bits, head, blk + kHeader);
    }
    for (int lane = 0; lane < kParts; lane++) crc ^= m6a_bgzf::crc_lane(crc_tab, in, n, lane);
    put_footer(blk + kHeader + body, crc, n);
    return total;
}

// blocks_host at level 1 or 2; n_by_type[t] grows by the blocks of BTYPE t
inline int64_t blocks_host(const uint8_t *text, int64_t n, int level, uint8_t *out, int64_t *n_by_type)
{
    uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; i++) crc_tab[i] = m6a_bgzf::crc_entry(i);
    uint16_t *tab = new uint16_t[kTableEntries];
    int64_t at = 0;
    for (int64_t off = 0; off < n; off += kBlockInput) {
        int btype;
        at += block_host(text + off, (int32_t)(n - off < kBlockInput ? n - off : kBlockInput), out + at, tab, crc_tab, level, &btype);
        if (n_by_type) ++n_by_type[btype];
    }
    delete[] tab;
    return at;
}

}  // namespace m6a_deflate

#ifdef M6A_DEFLATE_DEVICE_PART
// ---- part 2: kernels and the two entry points (inside m6a_prep.hip, behind m6a_csv.h: DevMem, PCHK, prep_fail, now_ms, g_d2h, Rounds
// and run_rounds are m6a_prep_kit.h's; CsvJob and the CSV writer's plan, launch and pwrite helpers are m6a_csv.h's) ----
namespace m6a_deflate {
namespace {

// The text of a round is two ranges of `text`: [0, n0) and [at1, at1 + n1) (the read rows and the site rows; n1 = 0 for one text).
// Each is cut into blocks of kBlockInput bytes, the first range's blocks first; a range ends its last block.
struct DeflText {
    const uint8_t *text;
    int64_t n0, at1, n1;
    __host__ __device__ int64_t blocks0() const { return n_blocks(n0); }
    __host__ __device__ int64_t blocks() const { return n_blocks(n0) + n_blocks(n1); }
    __device__ const uint8_t *block(int64_t b, int32_t *len) const
    {
        const int64_t b0 = blocks0(), base = b < b0 ? 0 : at1, n = b < b0 ? n0 : n1, off = (b < b0 ? b : b - b0) * kBlockInput;
        *len = (int32_t)(n - off < kBlockInput ? n - off : kBlockInput);
        return text + base + off;
    }
};

// status: [0] bytes of the first range's blocks, [1] bytes of all blocks, [2] stored blocks (zeroed before the launch)
__global__ void __launch_bounds__(kParts) bgzf_deflate_kernel(DeflText t, uint8_t *__restrict__ slots, int64_t *__restrict__ size,
                                                              unsigned long long *__restrict__ status)
{
    __shared__ uint16_t tab[kTableEntries];
    __shared__ uint32_t crc_tab[256], bits[kParts], head[kParts];
    const int lane = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    for (int i = lane; i < 256; i += kParts) crc_tab[i] = m6a_bgzf::crc_entry((uint32_t)i);
    int32_t n;
    const uint8_t *in = t.block(b, &n);
    uint8_t *out = slots + b * kSlot;
    uint32_t mine, first;
    part_bits(in, n, lane, tab, &mine, &first);
    bits[lane] = mine;
    head[lane] = first;
    __syncthreads();
    uint32_t incl = mine;
    for (int o = 1; o < kParts; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += v;
    }
    const uint32_t sum = (uint32_t)__shfl((int)incl, kParts - 1);
    bool stored;
    const int32_t body = stream_bytes(sum, n, &stored), total = kHeader + body + kFooter;
    if (stored) {
        if (lane == 0) put_stored_head(out + kHeader, n);
        for (int32_t i = lane; i < n; i += kParts) out[kHeader + 5 + i] = in[i];
    } else
        part_emit(in, n, lane, tab, incl - mine, bits, head, out + kHeader);
    uint32_t c = m6a_bgzf::crc_lane(crc_tab, in, n, lane);
    for (int o = kParts / 2; o > 0; o >>= 1) c ^= (uint32_t)__shfl_xor((int)c, o);
    if (lane == 0) {
        put_header(out, total);
        put_footer(out + kHeader + body, c, n);
        size[b] = total;
        if (stored) atomicAdd(status + 2, 1ull);
    }
}

struct LdsAdd {                            // a count in the wave's one histogram: an LDS integer atomic
    __device__ static void add(uint32_t *p) { atomicAdd(p, 1u); }
};

// Level 2: bgzf_deflate_kernel with the block's own codes.  The parts' tokens are counted into one histogram of the wave in LDS
// (kSymbols words) while their fixed-code strings are measured as at level 1; lane 0 runs the core's block_plan -- code lengths,
// canonical codes, the header, the three-way choice -- and the wave then measures and emits the parts under the codes that won.  A
// fixed or stored block costs the two walks of level 1, a dynamic block three.
// status as above, and [3] blocks of dynamic codes
__global__ void __launch_bounds__(kParts) bgzf_deflate_dyn_kernel(DeflText t, uint8_t *__restrict__ slots, int64_t *__restrict__ size,
                                                                  unsigned long long *__restrict__ status)
{
    __shared__ uint16_t tab[kTableEntries];
    __shared__ uint32_t crc_tab[256], bits[kParts], head[kParts], freq[kSymbols], work[kWork], plan[2];
    __shared__ Codes codes;
    __shared__ Header hdr;
    const int lane = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    for (int i = lane; i < 256; i += kParts) crc_tab[i] = m6a_bgzf::crc_entry((uint32_t)i);
    for (int i = lane; i < kSymbols; i += kParts) freq[i] = 0;
    __syncthreads();
    int32_t n;
    const uint8_t *in = t.block(b, &n);
    uint8_t *out = slots + b * kSlot;
    uint32_t mine, first, extra;
    part_hist<LdsAdd>(in, n, lane, tab, freq, &mine, &first, &extra);
    bits[lane] = mine;
    head[lane] = first;
    uint32_t incl = mine;
    for (int o = 1; o < kParts; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += v;
    }
    for (int o = kParts / 2; o > 0; o >>= 1) extra += (uint32_t)__shfl_xor((int)extra, o);
    const uint32_t fixed_bits = (uint32_t)__shfl((int)incl, kParts - 1);
    __syncthreads();
    if (lane == 0) {
        uint32_t hdr_bits;
        plan[0] = (uint32_t)block_plan(freq, extra, fixed_bits, n, codes, hdr, work, &hdr_bits);
        plan[1] = hdr_bits;
    }
    __syncthreads();
    const int btype = (int)plan[0];
    uint32_t base = 0;
    if (btype == 2) {
        part_bits_dyn(in, n, lane, tab, codes, &mine, &first);
        bits[lane] = mine;
        head[lane] = first;
        __syncthreads();
        incl = mine;
        for (int o = 1; o < kParts; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
            if (lane >= o) incl += v;
        }
        base = plan[1];
    }
    const uint32_t sum = base + (uint32_t)__shfl((int)incl, kParts - 1);
    const int32_t body = btype == 0 ? 5 + n : (int32_t)((sum + 7) >> 3), total = kHeader + body + kFooter;
    if (btype == 0) {
        if (lane == 0) put_stored_head(out + kHeader, n);
        for (int32_t i = lane; i < n; i += kParts) out[kHeader + 5 + i] = in[i];
    } else if (btype == 1)
        part_emit(in, n, lane, tab, incl - mine, bits, head, out + kHeader);
    else {
        if (lane == 0) header_emit(hdr, bits, head, out + kHeader);
        part_emit_dyn(in, n, lane, tab, codes, base + incl - mine, bits, head, out + kHeader);
    }
    uint32_t c = m6a_bgzf::crc_lane(crc_tab, in, n, lane);
    for (int o = kParts / 2; o > 0; o >>= 1) c ^= (uint32_t)__shfl_xor((int)c, o);
    if (lane == 0) {
        put_header(out, total);
        put_footer(out + kHeader + body, c, n);
        size[b] = total;
        if (btype == 0) atomicAdd(status + 2, 1ull);
        if (btype == 2) atomicAdd(status + 3, 1ull);
    }
}

// size[0, n) -> its exclusive sums in size[0, n], by one workgroup; the two totals into status
__global__ void __launch_bounds__(kBlk) bgzf_offsets_kernel(int64_t *__restrict__ size, int64_t n, int64_t n_first, unsigned long long *__restrict__ status)
{
    __shared__ int64_t part[kBlk];
    const int t = (int)threadIdx.x;
    const int64_t per = (n + kBlk - 1) / kBlk, lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; i++) sum += size[i];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < kBlk; i++) { const int64_t v = part[i]; part[i] = run; run += v; }
        size[n] = run;
        status[1] = (unsigned long long)run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t i = lo; i < hi; i++) { const int64_t v = size[i]; size[i] = run; run += v; }
    __syncthreads();
    if (t == 0) status[0] = (unsigned long long)size[n_first];
}

// block blockIdx.x from its slot to its offset in `packed`
__global__ void __launch_bounds__(kBlk) bgzf_pack_kernel(const uint8_t *__restrict__ slots, const int64_t *__restrict__ off, uint8_t *__restrict__ packed)
{
    const int64_t b = blockIdx.x, at = off[b];
    const int32_t len = (int32_t)(off[b + 1] - at);
    const uint8_t *src = slots + b * kSlot;
    for (int32_t i = (int32_t)threadIdx.x; i < len; i += kBlk) packed[at + i] = src[i];
}

// the three kernels on stream s (level 2: bgzf_deflate_dyn_kernel in the first one's place); `packed` may be the text's own buffer (it is read before it is written), with room for
// n0 + n1 + 64 bytes per block
inline int status_words(int level) { return level == 2 ? 4 : 3; }   // the record of a round

int deflate_launch(const DeflText &t, uint8_t *slots, int64_t *size, unsigned long long *status, uint8_t *packed, hipStream_t s, int level = 1)
{
    const int64_t nb = t.blocks();
    PCHK(hipMemsetAsync(status, 0, (size_t)status_words(level) * sizeof *status, s));
    if (!nb) return M6A_OK;
    if (nb > 0x7fffffffll) return prep_fail(M6A_EINVAL, "more than 2^31 BGZF blocks in a round");
    if (level == 2) bgzf_deflate_dyn_kernel<<<(unsigned)nb, kParts, 0, s>>>(t, slots, size, status);
    else bgzf_deflate_kernel<<<(unsigned)nb, kParts, 0, s>>>(t, slots, size, status);
    PCHK(hipGetLastError());
    bgzf_offsets_kernel<<<1, kBlk, 0, s>>>(size, nb, t.blocks0(), status);
    PCHK(hipGetLastError());
    bgzf_pack_kernel<<<(unsigned)nb, kBlk, 0, s>>>(slots, size, packed);
    PCHK(hipGetLastError());
    return M6A_OK;
}

inline int64_t packed_room(int64_t n0, int64_t n1) { return n0 + n1 + 64 * (n_blocks(n0) + n_blocks(n1)); }

int deflate_impl(int device_id, const uint8_t *text, int64_t n, int level, uint8_t *out, int64_t cap, int64_t *n_bytes, m6a_deflate_stats &st,
                 int64_t *n_by_type)
{
    DevMem m;
    int rc = open_device(device_id, m, "deflate it on the host, or in pieces");
    if (rc) return rc;
    g_d2h = 0;
    Streams S;
    PCHK(hipStreamCreateWithFlags(&S.s[0], hipStreamNonBlocking));
    hipStream_t s = S.s[0];
    const int64_t nb = n_blocks(n);
    uint8_t *dtext, *slots;
    int64_t *size;
    unsigned long long *status, h[4] = {0, 0, 0, 0};
    const int words = status_words(level);
    if ((rc = m.alloc(dtext, (size_t)packed_room(n, 0), "the text")) || (rc = m.alloc(slots, (size_t)(nb * kSlot), "BGZF slots")) ||
        (rc = m.alloc(size, (size_t)nb + 1, "BGZF sizes")) || (rc = m.alloc(status, (size_t)words, "flags")))
        return rc;
    if ((rc = h2d(dtext, text, (size_t)n, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    double t0 = now_ms();
    if ((rc = deflate_launch(DeflText{dtext, n, 0, 0}, slots, size, status, dtext, s, level)) || (rc = d2h(h, status, (size_t)words, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    st.ms_deflate = now_ms() - t0;
    st.n_blocks = nb;
    st.n_stored = (int64_t)h[2];
    if (n_by_type) {
        n_by_type[0] = (int64_t)h[2];
        n_by_type[2] = (int64_t)h[3];
        n_by_type[1] = nb - n_by_type[0] - n_by_type[2];
    }
    const int64_t total = (int64_t)h[1];
    *n_bytes = total + kEofBytes;
    if (cap < total + kEofBytes) return prep_fail(M6A_EINVAL, "the blocks take %lld bytes, the buffer holds %lld", (long long)(total + kEofBytes), (long long)cap);
    t0 = now_ms();
    if ((rc = d2h(out, dtext, (size_t)total, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    st.ms_copy = now_ms() - t0;
    for (int i = 0; i < kEofBytes; i++) out[total + i] = eof_byte(i);
    st.d2h_bytes = g_d2h;
    return M6A_OK;
}

struct DeflBufs {                          // beside a round's stream, events and pinned buffer (Rounds): its device buffers and status words
    uint8_t *text = nullptr, *slots = nullptr;
    int64_t *size = nullptr;
    unsigned long long *status = nullptr, *hstatus = nullptr;          // hstatus is pinned
    ~DeflBufs() { if (hstatus) (void)hipHostFree(hstatus); }
};

// the header line of a file as a BGZF block of its own, made by the host core at the writer's level
std::string header_block(const char *line, int32_t n, int level, int64_t *n_by_type)
{
    std::string blk((size_t)kSlot, '\0');
    blk.resize((size_t)blocks_host((const uint8_t *)line, n, level, (uint8_t *)&blk[0], n_by_type));
    return blk;
}

int csv_write_bgzf_impl(m6a_prep_sites &P, const char *out_dir, int write_header, int64_t n_limit, int n_threads, int level, m6a_csv_bgzf_stats &st,
                        int64_t *by_type)
{
    const int words = status_words(level);
    int64_t none[3], *const n_by_type = by_type ? by_type : none;
    n_by_type[0] = n_by_type[1] = n_by_type[2] = 0;
    CsvJob<m6a_csv_bgzf_stats> J(P, st);
    DeflBufs bufs[2];                                       // outlive the streams of rd
    Rounds rd;                                              // events: start, formatted, deflated, status copied, copy begins, copied
    int64_t cap_text = 0, cap_blocks = 0;
    int rc = J.begin(n_limit, n_threads, rd, 6, [&](int64_t ni, int64_t ns) {
        cap_text = std::max(cap_text, std::max(csv_align(ni) + ns, packed_room(ni, ns)));
        cap_blocks = std::max(cap_blocks, n_blocks(ni) + n_blocks(ns));
    });
    if (rc) return rc;
    const int64_t n_rounds = J.n_rounds();
    for (int i = 0; i < (n_rounds > 1 ? 2 : n_rounds ? 1 : 0); i++) {
        DeflBufs &r = bufs[i];
        if ((rc = J.m.alloc(r.text, (size_t)cap_text, "CSV text")) || (rc = J.m.alloc(r.slots, (size_t)(cap_blocks * kSlot), "BGZF slots")) ||
            (rc = J.m.alloc(r.size, (size_t)cap_blocks + 1, "BGZF sizes")) || (rc = J.m.alloc(r.status, (size_t)words, "flags")) ||
            (rc = rd.pinned(i, cap_text)))
            return rc;
        PCHK(hipHostMalloc((void **)&r.hstatus, (size_t)words * sizeof *r.hstatus, hipHostMallocDefault));
    }
    // the header line is a block of its own; appended to, an earlier end marker stays in the middle as an empty block
    if ((rc = J.open_files(out_dir, ".gz", write_header, [&](const char *line, int32_t n) { ++st.n_blocks; return header_block(line, n, level, n_by_type); })))
        return rc;
    const int64_t site0 = J.at_site, indiv0 = J.at_indiv;
    int64_t at_site = site0, at_indiv = indiv0;

    // ---- round k + 1 is formatted and deflated while round k is copied and written
    auto queue = [&](int64_t k) -> int {
        const int i = (int)(k & 1);
        DeflBufs &r = bufs[i];
        hipStream_t s = rd.s[i];
        const int64_t a = J.cut[(size_t)k], b = J.cut[(size_t)k + 1], ni = J.ni(a, b), ns = J.ns(a, b);
        PCHK(hipEventRecord(rd.e[i][0], s));
        int rc2 = csv_launch(J.d, J.plan, 0, a, b, (char *)r.text, csv_align(ni), s);
        if (rc2) return rc2;
        PCHK(hipEventRecord(rd.e[i][1], s));
        if ((rc2 = deflate_launch(DeflText{r.text, ni, csv_align(ni), ns}, r.slots, r.size, r.status, r.text, s, level))) return rc2;
        PCHK(hipEventRecord(rd.e[i][2], s));
        PCHK(hipMemcpyAsync(r.hstatus, r.status, (size_t)words * sizeof *r.status, hipMemcpyDeviceToHost, s));
        g_d2h += (int64_t)((size_t)words * sizeof *r.status);
        PCHK(hipEventRecord(rd.e[i][3], s));
        st.n_blocks += n_blocks(ni) + n_blocks(ns);
        return M6A_OK;
    };
    auto settle = [&](int64_t k) -> int {                   // the status words say how many bytes the payload copy takes
        const int i = (int)(k & 1);
        DeflBufs &r = bufs[i];
        PCHK(hipEventSynchronize(rd.e[i][3]));
        const int64_t a = J.cut[(size_t)k], b = J.cut[(size_t)k + 1], nb = n_blocks(J.ni(a, b)) + n_blocks(J.ns(a, b));
        const int64_t ct = (int64_t)r.hstatus[1], stored = (int64_t)r.hstatus[2], dyn = level == 2 ? (int64_t)r.hstatus[3] : 0;
        st.n_stored += stored;
        n_by_type[0] += stored;
        n_by_type[2] += dyn;
        n_by_type[1] += nb - stored - dyn;
        PCHK(hipEventRecord(rd.e[i][4], rd.s[i]));
        if (ct) PCHK(hipMemcpyAsync(rd.pin[i], r.text, (size_t)ct, hipMemcpyDeviceToHost, rd.s[i]));
        g_d2h += ct;
        PCHK(hipEventRecord(rd.e[i][5], rd.s[i]));
        return M6A_OK;
    };
    auto finish = [&](int64_t k) -> int {
        const int i = (int)(k & 1);
        PCHK(hipEventSynchronize(rd.e[i][5]));
        float fm = 0, dm = 0, cm = 0;
        PCHK(hipEventElapsedTime(&fm, rd.e[i][0], rd.e[i][1]));
        PCHK(hipEventElapsedTime(&dm, rd.e[i][1], rd.e[i][2]));
        PCHK(hipEventElapsedTime(&cm, rd.e[i][4], rd.e[i][5]));
        st.ms_format += fm;
        st.ms_deflate += dm;
        st.ms_copy += cm;
        const int64_t ci = (int64_t)bufs[i].hstatus[0], ct = (int64_t)bufs[i].hstatus[1];
        const double t0 = now_ms();
        if (!csv_pwrite_threads(J.g.fd, rd.pin[i], ci, at_indiv, J.nw)) return prep_fail(M6A_EIO, "cannot write %s", J.fi.c_str());
        if (!csv_pwrite_all(J.f.fd, rd.pin[i] + ci, ct - ci, at_site)) return prep_fail(M6A_EIO, "cannot write %s", J.fs.c_str());
        st.ms_write += now_ms() - t0;
        at_indiv += ci;
        at_site += ct - ci;
        return M6A_OK;
    };
    if ((rc = run_rounds(n_rounds, queue, settle, finish))) return rc;
    char eof[kEofBytes];
    for (int i = 0; i < kEofBytes; i++) eof[i] = (char)eof_byte(i);
    if (!csv_pwrite_all(J.f.fd, eof, kEofBytes, at_site)) return prep_fail(M6A_EIO, "cannot write %s", J.fs.c_str());
    if (!csv_pwrite_all(J.g.fd, eof, kEofBytes, at_indiv)) return prep_fail(M6A_EIO, "cannot write %s", J.fi.c_str());
    st.site_compressed = at_site + kEofBytes - (write_header ? 0 : site0);
    st.indiv_compressed = at_indiv + kEofBytes - (write_header ? 0 : indiv0);
    return J.close_files();
}

}  // namespace
}  // namespace m6a_deflate

extern "C" int m6a_bgzf_deflate_level(int device_id, const char *text, int64_t n, int level, char *out, int64_t cap, int64_t *n_bytes,
                                      m6a_deflate_stats *stats, int64_t n_by_type[3])
{
    if (!n_bytes || n < 0 || (n && !text)) return prep_fail(M6A_EINVAL, "null argument");
    if (level != 1 && level != 2) return prep_fail(M6A_EINVAL, "level %d: the BGZF writer has levels 1 and 2", level);
    *n_bytes = m6a_deflate::bound(n);
    if (stats) *stats = m6a_deflate_stats{};
    if (n_by_type) n_by_type[0] = n_by_type[1] = n_by_type[2] = 0;
    if (!out) return M6A_OK;                               // the sizing call
    m6a_deflate_stats st{};
    const int rc = guarded([&] { return m6a_deflate::deflate_impl(device_id, (const uint8_t *)text, n, level, (uint8_t *)out, cap, n_bytes, st, n_by_type); });
    if (stats) *stats = st;
    return rc;
}

extern "C" int m6a_bgzf_deflate(int device_id, const char *text, int64_t n, char *out, int64_t cap, int64_t *n_bytes, m6a_deflate_stats *stats)
{
    return m6a_bgzf_deflate_level(device_id, text, n, 1, out, cap, n_bytes, stats, nullptr);
}

extern "C" int m6a_prep_sites_write_csv_bgzf_level(m6a_prep_sites *p, const char *out_dir, int write_header, int64_t n_sites_limit, int n_threads,
                                                   int level, m6a_csv_bgzf_stats *stats, int64_t n_by_type[3])
{
    if (!p || !out_dir) return prep_fail(M6A_EINVAL, "null argument");
    if (level != 1 && level != 2) return prep_fail(M6A_EINVAL, "level %d: the BGZF writer has levels 1 and 2", level);
    if (n_by_type) n_by_type[0] = n_by_type[1] = n_by_type[2] = 0;
    m6a_csv_bgzf_stats st{};
    const int rc = guarded([&] { return m6a_deflate::csv_write_bgzf_impl(*p, out_dir, write_header, n_sites_limit, n_threads, level, st, n_by_type); });
    if (stats) *stats = st;
    return rc;
}

extern "C" int m6a_prep_sites_write_csv_bgzf(m6a_prep_sites *p, const char *out_dir, int write_header, int64_t n_sites_limit, int n_threads,
                                             m6a_csv_bgzf_stats *stats)
{
    return m6a_prep_sites_write_csv_bgzf_level(p, out_dir, write_header, n_sites_limit, n_threads, 1, stats, nullptr);
}
#endif  // M6A_DEFLATE_DEVICE_PART
#endif
