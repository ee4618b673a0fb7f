// m6a_bgzf.h -- BGZF (SAM specification section 4.1; include/m6a.h states the format) read for `eventalign_inference`.
//
// Part 1, the decode core: the block header walk, the bit reader, the Huffman table build, the symbol loop and every check, as plain
// C++ marked for host and device.  m6a_io.cpp compiles it for the CPU (m6a_io_bgzf_inflate: how the core is held to
// tests/bgzf_statement.py, malformed files included, under the sanitizers); m6a_prep.hip compiles the same text for gfx950.
// The three bounds hold by construction: every read of a block's input is `pos < n` checked in fill (past the end it reads zeros,
// and consuming one of those sets `over`), every write is checked against ISIZE before it happens, every distance against the bytes produced so far.  A
// malformed block is a reason code, never an out-of-range access.  The core is held to zlib in tests/test_bgzf_generated.py: on streams
// that tests/deflate_gen.py writes to cover RFC 1951 and on thousands of damaged ones, through m6a_io_bgzf_inflate and through
// tests/bgzf_core_main.cpp, a program of its own under ASan and UBSan that also feeds Walker in pieces of every size; the kernels
// see the same bytes in tests/test_gpu_bgzf_generated.py.
//
// Part 2 (M6A_BGZF_DEVICE_PART, m6a_prep.hip only): the kernels and the upload.
//   layout      one wave per BGZF block, four waves per workgroup.  The Huffman tables of a wave are 1.4 KB of LDS (canonical counts
//               + symbols, decoded a bit at a time as the statement does), so LDS never limits residency.  All 64 lanes run the symbol
//               loop with the same state: control flow is wave-uniform.  Lane 0 stores literals; a match of `len` bytes at `dist` is
//               copied by all lanes, byte i from out[pos - dist + i % dist] -- every source byte lies before pos, so a match needs no
//               step inside it, whatever the overlap.
//   visibility  the bytes a match loads were stored by this wave (lane 0's literals, any lane's earlier copies) earlier in program
//               order.  A CU's vector memory pipeline performs one wave's accesses in issue order, and a store updates the line in
//               that CU's L1; the workgroup-scope fence in front of the loads keeps the compiler from moving them and emits whatever
//               wait the target's memory model asks for between a store and a later load of the same workgroup.  No other wave, and
//               no other CU, reads a block's output before the kernel ends.
//   CRC-32      a second kernel, one wave per block: each lane takes 1/64 of the block's output through a byte table in LDS, its CRC
//               is advanced over the bytes behind it (a multiplication by x^(8 n) modulo the polynomial, zlib's crc32_combine), and the
//               64 terms are XORed.
//   status      both kernels atomicMin one 64-bit record, block << 8 | reason: the lowest bad block and, inside it, the first check
//               that failed (the CRC has the highest reason code).  8 bytes come back per file.
#ifndef M6A_BGZF_H
#define M6A_BGZF_H
#include <stdint.h>

#if defined(__HIPCC__)
#define M6A_HD __host__ __device__
#else
#define M6A_HD
#endif

namespace m6a_bgzf {

// reasons, in the order a block is checked; the texts are those of tests/bgzf_statement.py
enum {
    BR_OK = 0, BR_HEADER, BR_BSIZE, BR_ISIZE, BR_BTYPE, BR_STORED, BR_CODELEN, BR_SYMBOL, BR_DISTANCE, BR_OVERFLOW, BR_INPUT, BR_TRAILING, BR_LENGTH,
    BR_CRC, BR_COUNT
};
inline const char *reason_text(int r)
{
    static const char *const t[BR_COUNT] = {"ok", "bad header", "BSIZE runs past the end of the file", "ISIZE over 65536",
                                           "deflate block type 3", "stored LEN/NLEN mismatch", "invalid code lengths",
                                           "invalid literal/length or distance symbol", "distance reaches before the block's output",
                                           "output beyond ISIZE", "input exhausted before the end-of-block code",
                                           "deflate stream does not end at the footer", "inflated length is not ISIZE", "CRC-32 mismatch"};
    return r >= 0 && r < BR_COUNT ? t[r] : "?";
}

constexpr int32_t kMaxIsize = 65536;

// The header of the block at p, of which `have` bytes are there.  0: *total = BSIZE + 1 and *hdr = 12 + XLEN are set; > 0: that many
// bytes from p are needed before more can be said; < 0: -BR_HEADER.
M6A_HD inline int64_t block_header(const uint8_t *p, int64_t have, int32_t *total, int32_t *hdr)
{
    if (have < 12) return 12;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return -BR_HEADER;
    const int32_t end = 12 + (p[10] | p[11] << 8);
    if (have < end) return end;
    int32_t q = 12, bsize = -1;
    while (q + 4 <= end) {
        const int32_t slen = p[q + 2] | p[q + 3] << 8;
        if (q + 4 + slen > end) return -BR_HEADER;
        if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2 && bsize < 0) bsize = p[q + 4] | p[q + 5] << 8;
        q += 4 + slen;
    }
    if (q != end || bsize < 0 || bsize + 1 < end + 8) return -BR_HEADER;
    *total = bsize + 1;
    *hdr = end;
    return 0;
}

M6A_HD inline uint32_t le32(const uint8_t *p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

// ---- CRC-32 (reflected, polynomial 0xedb88320) ----
M6A_HD inline uint32_t crc_entry(uint32_t c)
{
    for (int k = 0; k < 8; k++) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1;
    return c;
}
M6A_HD inline uint32_t crc_bytes(const uint32_t *tab, const uint8_t *p, int32_t n)       // zlib's crc32(0, p, n)
{
    uint32_t c = 0xffffffffu;
    for (int32_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return ~c;
}
M6A_HD inline uint32_t crc_mul(uint32_t a, uint32_t b)             // a * b modulo the polynomial; bit 31 is x^0
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = b & 1 ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
M6A_HD inline uint32_t crc_xpow8(uint32_t n)                        // x^(8 n)
{
    uint32_t r = 0x80000000u, sq = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1) r = crc_mul(r, sq);
        sq = crc_mul(sq, sq);
    }
    return r;
}
// lane's term of the CRC of p[0, n) cut into 64 parts: the XOR of the 64 terms is crc32(0, p, n)
M6A_HD inline uint32_t crc_lane(const uint32_t *tab, const uint8_t *p, int32_t n, int lane)
{
    const int32_t per = (n + 63) / 64, lo = lane * per < n ? lane * per : n, hi = lo + per < n ? lo + per : n;
    if (hi <= lo) return 0;
    return crc_mul(crc_xpow8((uint32_t)(n - hi)), crc_bytes(tab, p + lo, hi - lo));
}

// ---- inflate (RFC 1951) ----
struct Bits {
    const uint8_t *in;
    int32_t n, pos;                 // pos: bytes taken into buf, those behind the input (read as zero) included
    uint32_t buf;
    int32_t cnt, pad;               // bits in buf; how many of them, at its top, stand for bytes behind the input
    bool over;                      // a bit behind the input was consumed
};
M6A_HD inline void fill(Bits &b, int need)                         // need <= 15
{
    while (b.cnt < need) {
        uint32_t byte = 0;
        if (b.pos < b.n) byte = b.in[b.pos];
        else b.pad += 8;
        b.pos++;
        b.buf |= byte << b.cnt;
        b.cnt += 8;
    }
}
M6A_HD inline void drop(Bits &b, int k)
{
    b.buf >>= k;
    b.cnt -= k;
    if (b.cnt < b.pad) b.over = true;
}
M6A_HD inline uint32_t getbits(Bits &b, int need)                  // need <= 15
{
    fill(b, need);
    const uint32_t v = b.buf & ((1u << need) - 1);
    drop(b, need);
    return v;
}
M6A_HD inline int32_t bytes_used(const Bits &b) { return b.pos - (b.cnt >> 3); }      // whole bytes consumed, the one in use included

struct Tables {                     // of one block being decoded: 1416 bytes
    uint16_t lcount[16], lsymbol[288], dcount[16], dsymbol[32], lengths[320], offs[16];
};

// canonical code from lengths[0, n): > 0 incomplete (unused codes), < 0 over-subscribed, 0 complete or no code at all; *max_len out
M6A_HD inline int construct(uint16_t *count, uint16_t *symbol, uint16_t *offs, const uint16_t *lengths, int n, int *max_len)
{
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (int s = 0; s < n; s++) count[lengths[s]]++;
    *max_len = 0;
    for (int l = 1; l < 16; l++)
        if (count[l]) *max_len = l;
    if (count[0] == n) return 0;
    int left = 1;
    for (int l = 1; l < 16; l++) {
        left = left * 2 - count[l];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int s = 0; s < n; s++)
        if (lengths[s]) symbol[offs[lengths[s]]++] = (uint16_t)s;
    return left;
}

// zlib's verdict (inflate_table) on a set: over-subscribed never; incomplete only as a single code of one bit, and never for the
// code-length code; no code at all passes here (zlib builds a table of invalid codes: using one is an error)
M6A_HD inline bool set_ok(int left, int max_len, bool codes) { return left == 0 || (left > 0 && !codes && max_len == 1); }

M6A_HD inline int decode(Bits &b, const uint16_t *count, const uint16_t *symbol)        // -1: no such code
{
    fill(b, 15);                                          // one refill, then the walk over the lengths in registers
    uint32_t bits = b.buf;
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; l++) {
        code |= (int)(bits & 1);
        bits >>= 1;
        const int c = count[l];
        if (code - c < first) {
            drop(b, l);
            return symbol[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    drop(b, 15);
    return -1;
}

M6A_HD inline void fixed_tables(Tables &T)
{
    int mx;
    for (int s = 0; s < 288; s++) T.lengths[s] = (uint16_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    construct(T.lcount, T.lsymbol, T.offs, T.lengths, 288, &mx);
    for (int s = 0; s < 30; s++) T.lengths[s] = 5;       // codes 30 and 31 stay unused: zlib calls them invalid
    construct(T.dcount, T.dsymbol, T.offs, T.lengths, 30, &mx);
}

M6A_HD inline int dynamic_tables(Bits &b, Tables &T)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const int nlen = (int)getbits(b, 5) + 257, ndist = (int)getbits(b, 5) + 1, ncode = (int)getbits(b, 4) + 4;
    if (b.over) return BR_INPUT;
    if (nlen > 286 || ndist > 30) return BR_CODELEN;
    for (int i = 0; i < 19; i++) T.lengths[order[i]] = (uint16_t)(i < ncode ? getbits(b, 3) : 0);
    if (b.over) return BR_INPUT;
    int mx, left = construct(T.lcount, T.lsymbol, T.offs, T.lengths, 19, &mx);
    if (!set_ok(left, mx, true) || mx == 0) return BR_CODELEN;
    for (int have = 0; have < nlen + ndist;) {
        const int sym = decode(b, T.lcount, T.lsymbol);
        if (b.over) return BR_INPUT;
        if (sym < 0) return BR_CODELEN;
        if (sym < 16) { T.lengths[have++] = (uint16_t)sym; continue; }
        int len = 0, rep;
        if (sym == 16) {
            if (have == 0) return BR_CODELEN;
            len = T.lengths[have - 1];
            rep = 3 + (int)getbits(b, 2);
        } else if (sym == 17) rep = 3 + (int)getbits(b, 3);
        else rep = 11 + (int)getbits(b, 7);
        if (b.over) return BR_INPUT;
        if (have + rep > nlen + ndist) return BR_CODELEN;
        while (rep--) T.lengths[have++] = (uint16_t)len;
    }
    if (T.lengths[256] == 0) return BR_CODELEN;            // no end-of-block code
    left = construct(T.dcount, T.dsymbol, T.offs, T.lengths + nlen, ndist, &mx);
    if (!set_ok(left, mx, false)) return BR_CODELEN;
    left = construct(T.lcount, T.lsymbol, T.offs, T.lengths, nlen, &mx);
    if (!set_ok(left, mx, false)) return BR_CODELEN;
    return BR_OK;
}

// Out: lit(pos, byte), copy(pos, dist, len) with dist <= pos, raw(pos, src, len); the caller has checked pos + len <= isize
template <class Out> M6A_HD inline int inflate(const uint8_t *in, int32_t n, Out &o, int32_t isize, Tables &T)
{
    Bits b{in, n, 0, 0, 0, 0, false};
    int32_t pos = 0;
    for (int last = 0; !last;) {
        last = (int)getbits(b, 1);
        const int type = (int)getbits(b, 2);
        if (b.over) return BR_INPUT;
        if (type == 3) return BR_BTYPE;
        if (type == 0) {
            b.pos = bytes_used(b);                        // the rest of the byte in use is dropped; whole bytes in buf go back
            b.buf = 0;
            b.cnt = b.pad = 0;
            if (b.pos + 4 > n) return BR_INPUT;
            const int32_t len = in[b.pos] | in[b.pos + 1] << 8, nlen = in[b.pos + 2] | in[b.pos + 3] << 8;
            if ((len ^ 0xffff) != nlen) return BR_STORED;
            b.pos += 4;
            if (b.pos + len > n) return BR_INPUT;
            if (pos + len > isize) return BR_OVERFLOW;
            o.raw(pos, in + b.pos, len);
            b.pos += len;
            pos += len;
            continue;
        }
        if (type == 1) fixed_tables(T);
        else {
            const int r = dynamic_tables(b, T);
            if (r) return r;
        }
        for (;;) {
            int sym = decode(b, T.lcount, T.lsymbol);
            if (b.over) return BR_INPUT;
            if (sym < 0) return BR_SYMBOL;
            if (sym < 256) {
                if (pos >= isize) return BR_OVERFLOW;
                o.lit(pos++, (uint8_t)sym);
                continue;
            }
            if (sym == 256) break;
            sym -= 257;
            if (sym >= 29) return BR_SYMBOL;               // 286, 287
            int32_t len;
            if (sym < 8) len = 3 + sym;
            else if (sym == 28) len = 258;
            else {
                const int ext = (sym >> 2) - 1;
                len = 3 + ((4 + (sym & 3)) << ext) + (int32_t)getbits(b, ext);
            }
            const int ds = decode(b, T.dcount, T.dsymbol);
            if (b.over) return BR_INPUT;
            if (ds < 0 || ds >= 30) return BR_SYMBOL;
            int32_t dist;
            if (ds < 4) dist = 1 + ds;
            else {
                const int ext = (ds >> 1) - 1;
                dist = 1 + ((2 + (ds & 1)) << ext) + (int32_t)getbits(b, ext);
            }
            if (b.over) return BR_INPUT;
            if (dist > pos) return BR_DISTANCE;
            if (pos + len > isize) return BR_OVERFLOW;
            o.copy(pos, dist, len);
            pos += len;
        }
    }
    if (bytes_used(b) != n) return BR_TRAILING;
    if (pos != isize) return BR_LENGTH;
    return BR_OK;
}

struct HostOut {
    uint8_t *out;
    void lit(int32_t pos, uint8_t v) { out[pos] = v; }
    void copy(int32_t pos, int32_t dist, int32_t len)
    {
        for (int32_t i = 0; i < len; i++) out[pos + i] = out[pos + i - dist];
    }
    void raw(int32_t pos, const uint8_t *src, int32_t len)
    {
        for (int32_t i = 0; i < len; i++) out[pos + i] = src[i];
    }
};

// The chain of a file that arrives in pieces (the upload's pinned chunks; a whole file is one piece).  feed() takes the next piece
// and calls `on_block(file offset, header bytes, total bytes, crc, isize)` for every block that is whole in what came so far; a block
// that straddles two pieces is carried.  It stops at the first bad header (`bad` = its reason, `bad_at` = its offset); finish() makes
// what is left at the end of the file an error too.
template <class F> struct Walker {
    F on_block;
    int64_t next = 0;               // file offset of the block not yet seen whole
    int bad = 0;
    int64_t bad_at = 0;
    uint8_t carry[65536 + 16];
    int64_t have = 0;               // bytes of the block at `next` held in carry
    explicit Walker(F f) : on_block(f) {}
    // what the block at p wants: 0 done (one block consumed, *used set), > 0 bytes needed in all, < 0 bad
    int64_t one(const uint8_t *p, int64_t avail, int64_t *used)
    {
        int32_t total = 0, hdr = 0;
        const int64_t r = block_header(p, avail, &total, &hdr);
        if (r < 0) { bad = (int)-r; bad_at = next; return -1; }
        if (r > 0) return r;
        if (avail < total) return total;
        const int32_t isize = (int32_t)le32(p + total - 4);
        if (le32(p + total - 4) > (uint32_t)kMaxIsize) { bad = BR_ISIZE; bad_at = next; return -1; }
        on_block(next, hdr, total, le32(p + total - 8), isize);
        *used = total;
        return 0;
    }
    void feed(const uint8_t *d, int64_t len)
    {
        int64_t at = 0, used = 0;
        while (!bad && at < len) {
            if (have) {                                   // finish the carried block first, taking only what it asks for
                const int64_t want = one(carry, have, &used);
                if (want < 0) return;
                if (want == 0) { next += used; have = 0; continue; }
                const int64_t take = want - have < len - at ? want - have : len - at;
                for (int64_t i = 0; i < take; i++) carry[have + i] = d[at + i];
                have += take;
                at += take;
                continue;                                 // (a block made whole by the piece's last byte is taken by the next call)
            }
            const int64_t want = one(d + at, len - at, &used);
            if (want < 0) return;
            if (want == 0) { next += used; at += used; continue; }
            for (int64_t i = 0; i < len - at; i++) carry[i] = d[at + i];      // want > len - at: at most 64 KiB
            have = len - at;
            at = len;
        }
    }
    void finish()
    {
        if (bad || !have) return;
        int64_t used = 0;
        const int64_t want = one(carry, have, &used);
        if (want == 0) { next += used; have = 0; return; }
        if (want < 0) return;
        int32_t total = 0, hdr = 0;
        bad = block_header(carry, have, &total, &hdr) == 0 ? BR_BSIZE : BR_HEADER;    // header whole, body cut: BSIZE; else the header is cut
        bad_at = next;
    }
};

}  // namespace m6a_bgzf

#ifdef M6A_BGZF_DEVICE_PART
// ---- part 2: kernels and the upload (inside m6a_prep.hip: DevMem, Streams, upload_range, PCHK, prep_fail, kBlk: m6a_prep_kit.h) ----
namespace {

struct BgzfBlock {                  // one block for the kernels: its deflate stream in the compressed buffer, its place in the text
    int64_t in_off, out_off;
    int32_t in_len, isize;
    uint32_t crc, pad;
};

struct WaveOut {
    uint8_t *out;
    int lane;
    __device__ void lit(int32_t pos, uint8_t v)
    {
        if (lane == 0) out[pos] = v;
    }
    __device__ void copy(int32_t pos, int32_t dist, int32_t len)
    {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");        // see `visibility` at the top
        for (int32_t i = lane; i < len; i += 64) out[pos + i] = out[pos - dist + i % dist];
    }
    __device__ void raw(int32_t pos, const uint8_t *src, int32_t len)
    {
        for (int32_t i = lane; i < len; i += 64) out[pos + i] = src[i];
    }
};

constexpr int kBgzfWaves = kBlk / 64;

__global__ void __launch_bounds__(kBlk) bgzf_inflate_kernel(const uint8_t *__restrict__ comp, const BgzfBlock *__restrict__ blk, int64_t nblk,
                                                            uint8_t *text, unsigned long long *__restrict__ bad)
{
    __shared__ m6a_bgzf::Tables T[kBgzfWaves];
    const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * kBgzfWaves + w;
    if (b >= nblk) return;
    const BgzfBlock B = blk[b];
    WaveOut o{text + B.out_off, lane};
    const int r = m6a_bgzf::inflate(comp + B.in_off, B.in_len, o, B.isize, T[w]);
    if (r && lane == 0) atomicMin(bad, (unsigned long long)b << 8 | (unsigned)r);
}

__global__ void __launch_bounds__(kBlk) bgzf_crc_kernel(const uint8_t *__restrict__ text, const BgzfBlock *__restrict__ blk, int64_t nblk,
                                                        unsigned long long *__restrict__ bad)
{
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = m6a_bgzf::crc_entry(threadIdx.x);
    __syncthreads();
    const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * kBgzfWaves + w;
    if (b >= nblk) return;
    const BgzfBlock B = blk[b];
    uint32_t c = m6a_bgzf::crc_lane(tab, text + B.out_off, B.isize, lane);
    for (int o = 32; o > 0; o >>= 1) c ^= (uint32_t)__shfl_xor((int)c, o);
    if (lane == 0 && c != B.crc) atomicMin(bad, (unsigned long long)b << 8 | (unsigned)m6a_bgzf::BR_CRC);
}

struct GatherRange { int64_t src, dst, len; };
// range blockIdx.x of the text, copied to its place in `out`
__global__ void gather_kernel(const uint8_t *__restrict__ f, const GatherRange *__restrict__ r, uint8_t *__restrict__ out)
{
    const GatherRange g = r[blockIdx.x];
    for (int64_t i = threadIdx.x; i < g.len; i += blockDim.x) out[g.dst + i] = f[g.src + i];
}

bool bgzf_is_gzip(int fd, int64_t n)
{
    uint8_t h[2] = {0, 0};
    return n >= 2 && ::pread(fd, h, 2, 0) == 2 && h[0] == 0x1f && h[1] == 0x8b;
}

struct BgzfUp {
    uint8_t *text = nullptr;        // in `m`, padded with zeros to whole 4 KB scan blocks
    int64_t n_text = 0, n_blocks = 0, comp_bytes = 0;
    double ms_upload = 0, ms_inflate = 0, ms_crc = 0;
};

// The compressed file [0, n) of fd goes up through S.pin (chunks of `chunk` bytes) while the host walks the block chain in the pinned
// bytes; the text buffer is allocated at the sum of ISIZE, every block inflated to its place and its CRC checked; the compressed
// buffer is released before this returns.  S.s[0] runs the kernels, S.s[1] the copies, as in front_half.
int bgzf_upload_inflate(int device_id, const char *path, int fd, int64_t n, DevMem &m, Streams &S, int64_t chunk, BgzfUp &U)
{
    int rc;
    uint8_t *dcomp;
    if ((rc = m.alloc(dcomp, (size_t)n, "the compressed file"))) return rc;
    std::vector<BgzfBlock> blocks;
    std::vector<int64_t> at;                              // file offset of every block, for the error text
    int64_t total = 0;
    auto on_block = [&](int64_t off, int32_t hdr, int32_t tot, uint32_t crc, int32_t isize) {
        blocks.push_back(BgzfBlock{off + hdr, total, tot - hdr - 8, isize, crc, 0});
        at.push_back(off);
        total += isize;
    };
    std::unique_ptr<m6a_bgzf::Walker<decltype(on_block)>> W(new m6a_bgzf::Walker<decltype(on_block)>(on_block));     // 64 KiB of carry
    const double t0 = now_ms();
    // the chain is walked while the chunk is on its way, and nothing goes up behind the first bad block; dcomp holds n bytes: no padding
    rc = upload_range(device_id, fd, path, S, dcomp, 0, n, chunk, [&](int slot, int64_t, int64_t len) {
        W->feed((const uint8_t *)S.pin[slot], len);
        return W->bad ? kUploadStop : (int)M6A_OK;
    }, false);
    if (rc) return rc;
    W->finish();
    U.ms_upload = now_ms() - t0;
    if (W->bad && W->bad_at == 0 && W->bad == m6a_bgzf::BR_HEADER)
        return prep_fail(M6A_EFORMAT, "%s is gzip but not BGZF: its first member has no BGZF header (compress it with `bgzip`, or "
                                      "`python -m m6anet_amd bgzip`)", path);
    const int64_t nblk = (int64_t)blocks.size(), nb = std::max<int64_t>(1, (total + kScanBytes - 1) / kScanBytes);
    U.n_text = total; U.n_blocks = nblk; U.comp_bytes = n;
    BgzfBlock *dblk;
    unsigned long long *dbad, hbad = ~0ull;
    if ((rc = m.alloc(U.text, (size_t)(nb * kScanBytes), "the file")) || (rc = m.alloc(dblk, (size_t)nblk + 1, "BGZF blocks")) ||
        (rc = m.alloc(dbad, 1, "flags")))
        return rc;
    hipStream_t s = S.s[0];
    if (nb * kScanBytes > total) PCHK(hipMemsetAsync(U.text + total, 0, (size_t)(nb * kScanBytes - total), s));
    PCHK(hipMemcpyAsync(dbad, &hbad, sizeof hbad, hipMemcpyHostToDevice, s));
    if (nblk) PCHK(hipMemcpyAsync(dblk, blocks.data(), (size_t)nblk * sizeof(BgzfBlock), hipMemcpyHostToDevice, s));
    const unsigned g = (unsigned)((nblk + kBgzfWaves - 1) / kBgzfWaves);
    double t1 = now_ms();
    if (nblk) {
        bgzf_inflate_kernel<<<g, kBlk, 0, s>>>(dcomp, dblk, nblk, U.text, dbad);
        PCHK(hipGetLastError());
    }
    PCHK(hipStreamSynchronize(s));
    U.ms_inflate = now_ms() - t1;
    t1 = now_ms();
    if (nblk) {
        bgzf_crc_kernel<<<g, kBlk, 0, s>>>(U.text, dblk, nblk, dbad);
        PCHK(hipGetLastError());
    }
    PCHK(hipMemcpyAsync(&hbad, dbad, sizeof hbad, hipMemcpyDeviceToHost, s));
    g_d2h += (int64_t)sizeof hbad;
    PCHK(hipStreamSynchronize(s));
    U.ms_crc = now_ms() - t1;
    if (hbad != ~0ull) {
        const int64_t b = (int64_t)(hbad >> 8);
        return prep_fail(M6A_EFORMAT, "%s: BGZF block at byte %lld: %s", path, (long long)at[(size_t)b], m6a_bgzf::reason_text((int)(hbad & 0xff)));
    }
    if (W->bad) return prep_fail(M6A_EFORMAT, "%s: BGZF block at byte %lld: %s", path, (long long)W->bad_at, m6a_bgzf::reason_text(W->bad));
    m.release(dcomp);
    m.release(dblk);
    m.release(dbad);
    return M6A_OK;
}

// front_half's BGZF branch: the text where the upload would have put it, and what the call reports
int bgzf_front(int device_id, const char *path, int fd, int64_t n_file, DevMem &m, Streams &S, int64_t chunk, uint8_t *&text, int64_t &n_text, Front &F, double *ms)
{
    BgzfUp U;
    const int rc = bgzf_upload_inflate(device_id, path, fd, n_file, m, S, chunk, U);
    if (rc) return rc;
    text = U.text;
    n_text = U.n_text;
    F.n_blocks = U.n_blocks;
    F.comp_bytes = U.comp_bytes;
    F.ms_inflate = U.ms_inflate + U.ms_crc;
    ms[0] = U.ms_upload;                                  // what crossed the link is the compressed file
    ms[5] = U.ms_upload > 0 ? (double)n_file / (U.ms_upload * 1e6) : 0;
    return M6A_OK;
}

}  // namespace

extern "C" int m6a_bgzf_inflate(int device_id, const char *path, char *text, int64_t cap, int64_t *n_bytes, m6a_bgzf_stats *stats)
{
    if (!path || !n_bytes) return prep_fail(M6A_EINVAL, "null argument");
    *n_bytes = 0;
    if (stats) *stats = m6a_bgzf_stats{};
    return guarded([&]() -> int {
        Fd fd;
        fd.fd = ::open(path, O_RDONLY);
        if (fd.fd < 0) return prep_fail(M6A_EIO, "cannot open %s", path);
        struct stat st;
        if (fstat(fd.fd, &st) != 0) return prep_fail(M6A_EIO, "cannot stat %s", path);
        const int64_t n = (int64_t)st.st_size;
        if (!bgzf_is_gzip(fd.fd, n)) return prep_fail(M6A_EFORMAT, "%s is not a gzip file", path);
        if (!text) {                                      // sizing: the chain alone, on the host
            int64_t total = 0;
            auto on_block = [&](int64_t, int32_t, int32_t, uint32_t, int32_t isize) { total += isize; };
            std::unique_ptr<m6a_bgzf::Walker<decltype(on_block)>> W(new m6a_bgzf::Walker<decltype(on_block)>(on_block));
            std::vector<uint8_t> buf((size_t)1 << 20);
            for (int64_t off = 0; off < n && !W->bad;) {
                const ssize_t r = ::pread(fd.fd, buf.data(), buf.size(), (off_t)off);
                if (r < 0 && errno == EINTR) continue;
                if (r <= 0) return prep_fail(M6A_EIO, "cannot read %s", path);
                W->feed(buf.data(), (int64_t)r);
                off += r;
            }
            W->finish();
            if (W->bad && W->bad_at == 0 && W->bad == m6a_bgzf::BR_HEADER)
                return prep_fail(M6A_EFORMAT, "%s is gzip but not BGZF: its first member has no BGZF header (compress it with `bgzip`, or "
                                              "`python -m m6anet_amd bgzip`)", path);
            *n_bytes = total;
            return M6A_OK;
        }
        DevMem m;
        int rc = open_device(device_id, m, "inflate it on the host");
        if (rc) return rc;
        g_d2h = 0;
        Streams S;
        int64_t chunk = 0;
        BgzfUp U;
        if ((rc = S.open((n + kScanBytes - 1) / kScanBytes * kScanBytes, chunk)) || (rc = bgzf_upload_inflate(device_id, path, fd.fd, n, m, S, chunk, U))) return rc;
        *n_bytes = U.n_text;
        if (cap < U.n_text) return prep_fail(M6A_EINVAL, "the text needs %lld bytes, the buffer holds %lld", (long long)U.n_text, (long long)cap);
        const double t0 = now_ms();
        if (U.n_text) PCHK(hipMemcpy(text, U.text, (size_t)U.n_text, hipMemcpyDeviceToHost));
        g_d2h += U.n_text;
        if (stats) *stats = m6a_bgzf_stats{U.n_blocks, U.comp_bytes, U.ms_upload, U.ms_inflate, U.ms_crc, now_ms() - t0, g_d2h};
        return M6A_OK;
    });
}

namespace {

// ranges of the text, packed end to end into `out` on the host (one kernel, one copy)
int bgzf_gather(DevMem &m, hipStream_t s, const uint8_t *text, int64_t n_text, const std::vector<int64_t> &src, const std::vector<int64_t> &len,
                std::vector<uint8_t> &out)
{
    std::vector<GatherRange> r(src.size());
    int64_t total = 0;
    for (size_t i = 0; i < src.size(); i++) {
        if (src[i] < 0 || len[i] < 0 || src[i] + len[i] > n_text) return prep_fail(M6A_EINVAL, "a byte range outside the inflated text");
        r[i] = GatherRange{src[i], total, len[i]};
        total += len[i];
    }
    out.resize((size_t)total);
    if (r.empty() || total == 0) return M6A_OK;
    int rc;
    GatherRange *dr;
    uint8_t *dout;
    if ((rc = m.alloc(dr, r.size(), "ranges")) || (rc = m.alloc(dout, (size_t)total, "ranges"))) return rc;
    PCHK(hipMemcpyAsync(dr, r.data(), r.size() * sizeof(GatherRange), hipMemcpyHostToDevice, s));
    gather_kernel<<<(unsigned)r.size(), kBlk, 0, s>>>(text, dr, dout);
    PCHK(hipGetLastError());
    PCHK(hipMemcpyAsync(out.data(), dout, (size_t)total, hipMemcpyDeviceToHost, s));
    g_d2h += total;
    PCHK(hipStreamSynchronize(s));
    m.release(dr);
    m.release(dout);
    return M6A_OK;
}

}  // namespace
#endif  // M6A_BGZF_DEVICE_PART
#endif
