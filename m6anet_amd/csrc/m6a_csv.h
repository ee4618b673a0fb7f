// m6a_csv.h -- data.site_proba.csv / data.indiv_proba.csv formatted on the device (include/m6a.h: m6a_csv_format,
// m6a_prep_sites_write_csv).  Part of m6a_prep.hip's translation unit (it works on that file's m6a_prep_sites handle and uses
// m6a_prep_kit.h's DevMem, scans, Rounds, run_rounds and error helpers); not a file to compile on its own.
//
// The bytes are the host writer's (m6a_io.cpp: format_rows, format_f16), i.e. the reference's '%s,%d,%s,%.16f,%s,%.16f' and
// '%s,%d,%s,%.16f' (m6anet/utils/inference_utils.py:62,66):
//   site row   <tx>,<pos>,<n_reads>,<%.16f of (double)site_prob>,<5-mer>,<%.16f of mod_ratio>\n
//   read row   <tx>,<pos>,<id>,<%.16f of (double)read_prob>\n      <id> = <int>.0 (one file) or <int>_<replicate> (pooled)
//              a handle built with read names (m6a_prep_sites_build_names): <id> = <uuid> or <uuid>_<replicate>, the 36 bytes
//              m6a_uuid.h formats from row <int> of the read's replicate's table
// Rows have different lengths, so a range of sites takes three steps:
//   lengths    csv_len_kernel, a wave per site: the length of its site row and the summed length of its read rows, and the count
//              of values the device DECLINES -- exactly these: a finite probability or ratio that is negative (-0.0 too) or >= 2;
//              a read id that is not integral, is negative (-0.0 too) or is >= 10^15 (the host prints those through str(float64))
//   offsets    exclusive 64-bit scans (scan_excl): every site's byte offset in either file, and both totals
//   write      csv_indiv_kernel, a wave per site, and csv_site_kernel, a wave per 64 sites.  A wave takes up to 64 consecutive rows
//              at a time -- as many as fit a tile of kCsvTile bytes of LDS: every lane formats its row into the tile at the row's
//              offset (lengths again, one wave scan), the tile shifted by the output's offset modulo 4 so that LDS dwords and global
//              dwords coincide; then consecutive lanes store consecutive aligned dwords, and only the first and the last dword of
//              a tile, which neighbours share, go out as byte stores.  A row longer than a tile (a transcript name of ~8 KB) is
//              written by its lane straight to global memory.
// '%.16f' of 0 <= v < 2 is the host's method: v = m 2^e exactly, n = round-half-even(m 10^16 / 2^-e) from one 128-bit product,
// then 1 + 16 digits (n <= 2 10^16 fits 64 bits: no 128-bit division).  NaN and infinities print as glibc prints them: nan, -nan,
// inf, -inf.
//
// m6a_prep_sites_write_csv: lengths and offsets for the whole job first (both file sizes, every round's offsets and the declined
// count are known before a file is opened), then rounds of whole sites bounded by M6A_CSV_ROUND_KB of text (default 32768; a site
// with more text than that is a round of its own, and the buffers are sized for the largest round), double-buffered: round k + 1 is
// formatted and copied into its pinned buffer on one stream while round k is pwrite()n at its offsets by n_threads threads.
#pragma once

#include <atomic>
#include <thread>

#include "m6a_host_cpus.h"

namespace {

constexpr int kCsvWave = 64;               // threads per block of the CSV kernels: one wave
constexpr int kCsvTile = 8192;             // bytes of text a wave stages in LDS at a time
constexpr int64_t kCsvRoundKB = 32768;     // default M6A_CSV_ROUND_KB

struct CsvDev {                            // device pointers; sites and reads are indexed as in the job
    const int64_t *off;                    // [S + 1]
    const uint32_t *site_tx;               // [S]
    const int64_t *site_pos;               // [S]
    const uint8_t *kmer;                   // 5-mer of site i: kmer[i * kstride + kofs .. + 5)
    int kstride, kofs;
    const uint8_t *tx_blob;
    const int64_t *tx_off;                 // [n_tx + 1]
    const double *ids;                     // [R]
    const int32_t *read_rep;               // [R] replicate of each read, or null:
    const int32_t *part_cnt;               // [S][K] reads of each site by replicate, in replicate order (K > 1, read_rep null)
    int K;                                 // replicates; 1: ids print as <int>.0
    const float *read_prob, *site_prob;    // [R], [S]
    const double *mod_ratio;               // [S]
    const uint8_t *names16;                // read names, 16 bytes each, or null: replicate f's are rows [name_off[f], name_off[f + 1])
    const int64_t *name_off;               // [K + 1]
};

__device__ inline int csv_digits(uint64_t v)
{
    int n = 1;
    for (uint64_t p = 10; n < 20 && v >= p; p *= 10) ++n;
    return n;
}

__device__ inline void csv_put_u64(char *o, uint64_t v, int nd)
{
    int i = nd;
    while (v > 0xffffffffull) { const uint64_t q = v / 10; o[--i] = (char)('0' + (int)(v - q * 10)); v = q; }
    uint32_t w = (uint32_t)v;
    while (i > 0) { const uint32_t q = w / 10; o[--i] = (char)('0' + (int)(w - q * 10)); w = q; }
}

__device__ inline int csv_i64_len(int64_t v) { return v < 0 ? 1 + csv_digits(0 - (uint64_t)v) : csv_digits((uint64_t)v); }

__device__ inline int csv_put_i64(char *o, int64_t v)
{
    int k = 0;
    uint64_t u = (uint64_t)v;
    if (v < 0) { o[k++] = '-'; u = 0 - u; }
    const int nd = csv_digits(u);
    csv_put_u64(o + k, u, nd);
    return k + nd;
}

// '%.16f' of the double with these bits: its length, and whether the device declines it
__device__ inline int csv_f16_len(uint64_t bits, unsigned &declined)
{
    const int be = (int)(bits >> 52) & 0x7ff;
    if (be == 0x7ff) return (bits >> 63) ? 4 : 3;          // nan, inf / -nan, -inf
    if ((bits >> 63) || be >= 1024) declined++;            // negative (-0.0 too) or >= 2
    return 18;
}

__device__ inline int csv_put_f16(char *o, uint64_t bits)
{
    const int be = (int)(bits >> 52) & 0x7ff;
    uint64_t m = bits & ((1ull << 52) - 1);
    if (be == 0x7ff) {
        int k = 0;
        if (bits >> 63) o[k++] = '-';
        o[k++] = m ? 'n' : 'i';
        o[k++] = m ? 'a' : 'n';
        o[k++] = m ? 'n' : 'f';
        return k;
    }
    uint64_t n = 0;                                         // round_half_even(v * 1e16) <= 2e16
    if (!(bits >> 63) && be < 1024) {                       // (a declined value is never written out; its 18 bytes stay in bounds)
        int e;                                              // v = m * 2^e
        if (be == 0) e = -1074; else { m |= 1ull << 52; e = be - 1075; }
        const unsigned __int128 prod = (unsigned __int128)m * 10000000000000000ull;
        const int sh = -e;                                  // >= 52
        if (sh < 108) {                                     // else prod < 2^107 is below one half
            n = (uint64_t)(prod >> sh);
            const unsigned __int128 rem = prod & (((unsigned __int128)1 << sh) - 1), half = (unsigned __int128)1 << (sh - 1);
            if (rem > half || (rem == half && (n & 1))) n++;
        }
    }
    const uint64_t kE16 = 10000000000000000ull;
    const int ip = n >= 2 * kE16 ? 2 : n >= kE16 ? 1 : 0;
    const uint64_t fp = n - (uint64_t)ip * kE16;
    const uint32_t hi = (uint32_t)(fp / 100000000ull), lo = (uint32_t)(fp - (uint64_t)hi * 100000000ull);
    o[0] = (char)('0' + ip);
    o[1] = '.';
    csv_put_u64(o + 2, hi, 8);
    csv_put_u64(o + 10, lo, 8);
    return 18;
}

// a read id the device prints: integral, sign bit clear, below 10^15
__device__ inline bool csv_id_ok(double id) { return id == floor(id) && !(__double_as_longlong(id) >> 63 & 1) && id < 1e15; }

__device__ inline int csv_read_rep(const CsvDev &d, int64_t site, int64_t r, int64_t j)
{
    if (d.read_rep) return d.read_rep[r];
    int f = 0;
    for (; f < d.K - 1; f++) {
        const int64_t c = d.part_cnt[site * d.K + f];
        if (j < c) break;
        j -= c;
    }
    return f;
}

// the rows of one site in data.indiv_proba.csv
struct CsvReadRows {
    const CsvDev &d;
    int64_t site, r0, pos, name_len;
    const uint8_t *name;
    int head_len;                                           // the ",<pos>," after the name

    __device__ CsvReadRows(const CsvDev &d_, int64_t i) : d(d_), site(i)
    {
        r0 = d.off[i];
        pos = d.site_pos[i];
        const int64_t t0 = d.tx_off[d.site_tx[i]];
        name = d.tx_blob + t0;
        name_len = d.tx_off[d.site_tx[i] + 1] - t0;
        head_len = 2 + csv_i64_len(pos);
    }
    // the table row of read r's name, or -1: the id is not an index into its replicate's table (the build makes none such)
    __device__ int64_t name_row(double id, int rep) const
    {
        if (!csv_id_ok(id)) return -1;
        const int64_t k = d.name_off[rep] + (int64_t)id;
        return k < d.name_off[rep + 1] ? k : -1;
    }
    __device__ int64_t len(int64_t j, unsigned &declined) const
    {
        const int64_t r = r0 + j;
        const double id = d.ids[r];
        int n;
        if (d.names16) {
            const int rep = d.K > 1 ? csv_read_rep(d, site, r, j) : 0;
            if (name_row(id, rep) < 0) declined++;
            n = m6a_uuid::kLen + (d.K > 1 ? 1 + csv_digits((uint64_t)rep) : 0);
        } else {
            const bool ok = csv_id_ok(id);
            if (!ok) declined++;
            n = csv_digits(ok ? (uint64_t)id : 0);
            n += d.K > 1 ? 1 + csv_digits((uint64_t)csv_read_rep(d, site, r, j)) : 2;
        }
        n += 2 + csv_f16_len((uint64_t)__double_as_longlong((double)d.read_prob[r]), declined);
        return name_len + head_len + n;
    }
    __device__ int64_t len(int64_t j) const { unsigned x = 0; return len(j, x); }
    __device__ void put(int64_t j, char *o) const
    {
        const int64_t r = r0 + j;
        for (int64_t c = 0; c < name_len; c++) o[c] = (char)name[c];
        o += name_len;
        *o++ = ',';
        o += csv_put_i64(o, pos);
        *o++ = ',';
        const double id = d.ids[r];
        if (d.names16) {
            const int64_t k = name_row(id, d.K > 1 ? csv_read_rep(d, site, r, j) : 0);
            const m6a_uuid::Name nm = k < 0 ? m6a_uuid::Name{0, 0} : m6a_uuid::from_bytes(d.names16 + k * 16);
            m6a_uuid::format(nm.hi, nm.lo, o);
            o += m6a_uuid::kLen;
        } else {
            const uint64_t u = csv_id_ok(id) ? (uint64_t)id : 0;
            const int nd = csv_digits(u);
            csv_put_u64(o, u, nd);
            o += nd;
        }
        if (d.K > 1) {
            *o++ = '_';
            const uint64_t rep = (uint64_t)csv_read_rep(d, site, r, j);
            const int nr = csv_digits(rep);
            csv_put_u64(o, rep, nr);
            o += nr;
        } else if (!d.names16) {
            *o++ = '.';
            *o++ = '0';
        }
        *o++ = ',';
        o += csv_put_f16(o, (uint64_t)__double_as_longlong((double)d.read_prob[r]));
        *o = '\n';
    }
};

// the rows of data.site_proba.csv from site `first` on
struct CsvSiteRows {
    const CsvDev &d;
    int64_t first;

    __device__ int64_t len(int64_t j, unsigned &declined) const
    {
        const int64_t i = first + j;
        const uint32_t t = d.site_tx[i];
        int64_t n = d.tx_off[t + 1] - d.tx_off[t];
        n += 1 + csv_i64_len(d.site_pos[i]) + 1 + csv_digits((uint64_t)(d.off[i + 1] - d.off[i])) + 1;
        n += csv_f16_len((uint64_t)__double_as_longlong((double)d.site_prob[i]), declined) + 1 + 5 + 1;
        n += csv_f16_len((uint64_t)__double_as_longlong(d.mod_ratio[i]), declined) + 1;
        return n;
    }
    __device__ int64_t len(int64_t j) const { unsigned x = 0; return len(j, x); }
    __device__ void put(int64_t j, char *o) const
    {
        const int64_t i = first + j;
        const int64_t t0 = d.tx_off[d.site_tx[i]], nl = d.tx_off[d.site_tx[i] + 1] - t0;
        for (int64_t c = 0; c < nl; c++) o[c] = (char)d.tx_blob[t0 + c];
        o += nl;
        *o++ = ',';
        o += csv_put_i64(o, d.site_pos[i]);
        *o++ = ',';
        const uint64_t n = (uint64_t)(d.off[i + 1] - d.off[i]);
        const int nd = csv_digits(n);
        csv_put_u64(o, n, nd);
        o += nd;
        *o++ = ',';
        o += csv_put_f16(o, (uint64_t)__double_as_longlong((double)d.site_prob[i]));
        *o++ = ',';
        for (int c = 0; c < 5; c++) *o++ = (char)d.kmer[i * d.kstride + d.kofs + c];
        *o++ = ',';
        o += csv_put_f16(o, (uint64_t)__double_as_longlong(d.mod_ratio[i]));
        *o = '\n';
    }
};

// One wave writes rows [0, n_rows) of `R`, back to back from out[g0] on.  `out` is 4-byte aligned.
template <class Rows>
__device__ void csv_emit(char *__restrict__ out, int64_t g0, int64_t n_rows, const Rows &R, uint32_t *lds)
{
    const int lane = (int)threadIdx.x;
    char *l8 = (char *)lds;
    for (int64_t rb = 0; rb < n_rows;) {                    // rb and g0 are the same in every lane
        const int64_t row = rb + lane;
        const int64_t len = row < n_rows ? R.len(row) : 0;
        int64_t incl = len;
        for (int o = 1; o < kCsvWave; o <<= 1) {
            const int64_t t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        const int pad = (int)(g0 & 3);
        const bool fits = row < n_rows && pad + incl <= kCsvTile;
        const unsigned long long mask = __ballot(fits);     // lengths are positive: the rows that fit are the first k
        const int k = ~mask ? __builtin_ctzll(~mask) : kCsvWave;
        if (k == 0) {                                       // row rb is longer than a tile: straight to global memory
            if (lane == 0) R.put(row, out + g0);
            g0 += __shfl(len, 0);
            rb += 1;
            continue;
        }
        if (lane < k) R.put(row, l8 + pad + (incl - len));
        const int end = pad + (int)__shfl(incl, k - 1);
        __syncthreads();
        char *ga = out + (g0 - pad);
        for (int b0 = lane * 4; b0 < end; b0 += kCsvWave * 4) {
            if (b0 >= pad && b0 + 4 <= end) *(uint32_t *)(ga + b0) = lds[b0 >> 2];
            else
                for (int b = b0 < pad ? pad : b0; b < b0 + 4 && b < end; b++) ga[b] = l8[b];
        }
        __syncthreads();
        g0 += end - pad;
        rb += k;
    }
}

// lengths of sites [a, b): len[i - a] for either file, and the declined values counted
__global__ __launch_bounds__(kCsvWave) void csv_len_kernel(CsvDev d, int64_t a, int64_t b, int64_t *__restrict__ site_len,
                                                           int64_t *__restrict__ indiv_len, unsigned long long *__restrict__ declined)
{
    const int64_t i = a + blockIdx.x;
    if (i >= b) return;
    const int lane = (int)threadIdx.x;
    const CsvReadRows rows(d, i);
    const int64_t n = d.off[i + 1] - rows.r0;
    int64_t sum = 0;
    unsigned decl = 0;
    for (int64_t j = lane; j < n; j += kCsvWave) sum += rows.len(j, decl);
    if (lane == 0) site_len[i - a] = CsvSiteRows{d, i}.len(0, decl);
    for (int o = kCsvWave / 2; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        decl += __shfl_xor(decl, o);
    }
    if (lane == 0) {
        indiv_len[i - a] = sum;
        if (decl) atomicAdd(declined, (unsigned long long)decl);
    }
}

// indiv_off / site_off: the scanned lengths of sites [A, ...); text of sites [a, b) lands in `out` from byte 0 on
__global__ __launch_bounds__(kCsvWave) void csv_indiv_kernel(CsvDev d, int64_t A, int64_t a, int64_t b, const int64_t *__restrict__ indiv_off,
                                                             char *__restrict__ out)
{
    __shared__ uint32_t lds[(kCsvTile + 8) / 4];
    const int64_t i = a + blockIdx.x;
    if (i >= b) return;
    const CsvReadRows rows(d, i);
    csv_emit(out, indiv_off[i - A] - indiv_off[a - A], d.off[i + 1] - rows.r0, rows, lds);
}

__global__ __launch_bounds__(kCsvWave) void csv_site_kernel(CsvDev d, int64_t A, int64_t a, int64_t b, const int64_t *__restrict__ site_off,
                                                            char *__restrict__ out)
{
    __shared__ uint32_t lds[(kCsvTile + 8) / 4];
    const int64_t i = a + (int64_t)blockIdx.x * kCsvWave;
    if (i >= b) return;
    csv_emit(out, site_off[i - A] - site_off[a - A], b - i < kCsvWave ? b - i : (int64_t)kCsvWave, CsvSiteRows{d, i}, lds);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

// lengths and offsets of sites [A, B): the scanned arrays on the device (B - A + 1 entries, the last one the total) and on the host
struct CsvPlan {
    int64_t *d_site = nullptr, *d_indiv = nullptr;
    std::vector<int64_t> site, indiv;
    int64_t declined = 0;
};

int csv_plan(DevMem &m, const CsvDev &d, int64_t A, int64_t B, hipStream_t s, CsvPlan &P)
{
    const int64_t n = B - A;
    if (n > 0x7fffffffll) return prep_fail(M6A_EINVAL, "more than 2^31 sites");
    unsigned long long *dd, hd = 0;
    int rc;
    if ((rc = m.alloc(P.d_site, (size_t)n + 1, "CSV offsets")) || (rc = m.alloc(P.d_indiv, (size_t)n + 1, "CSV offsets")) ||
        (rc = m.alloc(dd, 1, "flags")))
        return rc;
    PCHK(hipMemsetAsync(dd, 0, sizeof *dd, s));
    PCHK(hipMemsetAsync(P.d_site + n, 0, sizeof(int64_t), s));
    PCHK(hipMemsetAsync(P.d_indiv + n, 0, sizeof(int64_t), s));
    if (n) {
        csv_len_kernel<<<(unsigned)n, kCsvWave, 0, s>>>(d, A, B, P.d_site, P.d_indiv, dd);
        PCHK(hipGetLastError());
    }
    if ((rc = scan_excl(m, P.d_site, n + 1, s)) || (rc = scan_excl(m, P.d_indiv, n + 1, s))) return rc;
    P.site.resize((size_t)n + 1);
    P.indiv.resize((size_t)n + 1);
    if ((rc = d2h(P.site.data(), P.d_site, (size_t)n + 1, s)) || (rc = d2h(P.indiv.data(), P.d_indiv, (size_t)n + 1, s)) || (rc = d2h(&hd, dd, 1, s)))
        return rc;
    PCHK(hipStreamSynchronize(s));
    P.declined = (int64_t)hd;
    return M6A_OK;
}

int csv_declined(int64_t n)
{
    return prep_fail(M6A_EDECLINED, "%lld values are outside what the device formats (a probability or ratio that is negative or >= 2, "
                     "a read index that is not an integer in [0, 10^15))", (long long)n);
}

// the text of sites [a, b) of a plan over [A, ...): the read rows from out[0] on, the site rows from out[site_at] on
int csv_launch(const CsvDev &d, const CsvPlan &P, int64_t A, int64_t a, int64_t b, char *out, int64_t site_at, hipStream_t s)
{
    if (b <= a) return M6A_OK;
    csv_indiv_kernel<<<(unsigned)(b - a), kCsvWave, 0, s>>>(d, A, a, b, P.d_indiv, out);
    PCHK(hipGetLastError());
    csv_site_kernel<<<(unsigned)((b - a + kCsvWave - 1) / kCsvWave), kCsvWave, 0, s>>>(d, A, a, b, P.d_site, out + site_at);
    PCHK(hipGetLastError());
    return M6A_OK;
}

inline int64_t csv_align(int64_t n) { return (n + 255) & ~(int64_t)255; }

bool csv_pwrite_all(int fd, const char *p, int64_t n, int64_t at)
{
    while (n) {
        const ssize_t w = ::pwrite(fd, p, (size_t)n, (off_t)at);
        if (w < 0) { if (errno == EINTR) continue; return false; }
        p += w; n -= w; at += w;
    }
    return true;
}

// `n` bytes at file offset `at`, cut into pieces of at least 1 MB for up to `nw` threads
bool csv_pwrite_threads(int fd, const char *p, int64_t n, int64_t at, int nw)
{
    const int pieces = (int)std::max<int64_t>(1, std::min<int64_t>(nw, n >> 20));
    if (pieces == 1) return csv_pwrite_all(fd, p, n, at);
    std::atomic<bool> ok{true};
    std::vector<std::thread> th;
    const int64_t per = (n + pieces - 1) / pieces;
    auto work = [&](int w) {
        const int64_t b0 = std::min<int64_t>(n, per * w), b1 = std::min<int64_t>(n, b0 + per);
        if (!csv_pwrite_all(fd, p + b0, b1 - b0, at + b0)) ok = false;
    };
    for (int w = 1; w < pieces; w++) th.emplace_back(work, w);
    work(0);
    for (auto &t : th) t.join();
    return ok;
}

const char kCsvSiteHeader[] = "transcript_id,transcript_position,n_reads,probability_modified,kmer,mod_ratio\n";
const char kCsvIndivHeader[] = "transcript_id,transcript_position,read_index,probability_modified\n";

const char kCsvAdvice[] = "write the CSV files on the host (--csv host)";

// whatever way a writer's call ends, what it copied and allocated is reported
template <class Stats> struct Account {
    m6a_prep_sites &P; DevMem &m; Stats &st;
    ~Account()
    {
        st.d2h_bytes = g_d2h;
        P.info.d2h_bytes += g_d2h;
        P.info.peak_bytes = std::max<int64_t>(P.info.peak_bytes, (int64_t)(P.held + m.peak));
    }
};

// What m6a_prep_sites_write_csv and its BGZF twin (m6a_deflate.h) do around their rounds.  begin: the device, the small uploads, the
// lengths and offsets of the whole job, the refusal of a declined value, the rounds.  The writer then allocates every device and pinned
// buffer, so that a call over the budget touches no file, and only then open_files; close_files after the last round.
template <class Stats> struct CsvJob {
    m6a_prep_sites &P;
    Stats &st;
    DevMem m;
    Account<Stats> account{P, m, st};
    int64_t S = 0;
    int nw = 0;
    CsvDev d{};
    CsvPlan plan;
    std::vector<int64_t> cut{0};            // round k is sites [cut[k], cut[k + 1])
    std::string fs, fi;
    Fd f, g;
    int64_t at_site = 0, at_indiv = 0;      // where the rows begin in either file
    CsvJob(m6a_prep_sites &P_, Stats &st_) : P(P_), st(st_) {}
    int64_t ni(int64_t a, int64_t b) const { return plan.indiv[(size_t)b] - plan.indiv[(size_t)a]; }
    int64_t ns(int64_t a, int64_t b) const { return plan.site[(size_t)b] - plan.site[(size_t)a]; }
    int64_t n_rounds() const { return (int64_t)cut.size() - 1; }

    // on_round(ni, ns) sees the read and site text of every round: the writer sizes its buffers from them
    template <class OnRound> int begin(int64_t n_limit, int n_threads, Rounds &rd, int n_events, OnRound on_round)
    {
        g_d2h = 0;
        const m6a_prep_sites_info &I = P.info;
        S = n_limit >= 0 ? std::min<int64_t>(n_limit, I.n_sites) : I.n_sites;
        if (I.n_sites && !P.csv_ids) return prep_fail(M6A_EINVAL, "the handle holds no read ids on the device");
        nw = n_threads > 0 ? n_threads : m6a_usable_cpus();
        int rc;
        if ((rc = open_device(P.device, m, kCsvAdvice)) || (rc = rd.open(n_events))) return rc;
        hipStream_t s = rd.s[0];
        uint8_t *blob;
        int64_t *tx_off;
        const size_t nblob = (size_t)(I.n_tx ? I.tx_off[I.n_tx] : 0);
        if ((rc = m.alloc(blob, nblob + 1, "transcript names")) || (rc = m.alloc(tx_off, (size_t)I.n_tx + 1, "transcript names"))) return rc;
        if ((rc = h2d(blob, (const uint8_t *)I.tx_blob, nblob, s)) || (rc = h2d(tx_off, I.tx_off, I.n_tx ? (size_t)I.n_tx + 1 : 0, s))) return rc;
        d = CsvDev{I.off, P.csv_tx, P.csv_pos, P.csv_k7, 7, 1, blob, tx_off, P.csv_ids, nullptr, I.n_rep > 1 ? P.csv_parts : nullptr,
                   I.n_rep > 1 ? I.n_rep : 1, I.read_prob, I.site_prob, I.mod_ratio, P.csv_names, P.csv_name_off};
        const double t0 = now_ms();
        if ((rc = csv_plan(m, d, 0, S, s, plan))) return rc;
        st.ms_format += now_ms() - t0;
        st.n_declined = plan.declined;
        st.site_bytes = plan.site[(size_t)S];
        st.indiv_bytes = plan.indiv[(size_t)S];
        if (plan.declined) return csv_declined(plan.declined);
        m6a_rounds::cut_rounds(S, round_kb("M6A_CSV_ROUND_KB", kCsvRoundKB) << 10, [&](int64_t a, int64_t b) { return ni(a, b) + ns(a, b); },
                               [&](int64_t a, int64_t b) { cut.push_back(b); on_round(ni(a, b), ns(a, b)); });
        st.n_rounds = n_rounds();
        return M6A_OK;
    }

    // both files of out_dir; header(line, n) gives the bytes that stand for a header line.  write_header = 0 appends: nothing is
    // truncated and the rows go behind whatever the files hold
    template <class Header> int open_files(const char *out_dir, const char *suffix, int write_header, Header header)
    {
        fs = std::string(out_dir) + "/data.site_proba.csv" + suffix;
        fi = std::string(out_dir) + "/data.indiv_proba.csv" + suffix;
        const int flags = O_WRONLY | O_CREAT | (write_header ? O_TRUNC : 0);
        f.fd = ::open(fs.c_str(), flags, 0644);
        if (f.fd < 0) return prep_fail(M6A_EIO, "cannot open %s", fs.c_str());
        g.fd = ::open(fi.c_str(), flags, 0644);
        if (g.fd < 0) return prep_fail(M6A_EIO, "cannot open %s", fi.c_str());
        if (write_header) {
            const std::string hs = header(kCsvSiteHeader, (int32_t)sizeof(kCsvSiteHeader) - 1), hi = header(kCsvIndivHeader, (int32_t)sizeof(kCsvIndivHeader) - 1);
            at_site = (int64_t)hs.size();
            at_indiv = (int64_t)hi.size();
            if (!csv_pwrite_all(f.fd, hs.data(), at_site, 0)) return prep_fail(M6A_EIO, "cannot write %s", fs.c_str());
            if (!csv_pwrite_all(g.fd, hi.data(), at_indiv, 0)) return prep_fail(M6A_EIO, "cannot write %s", fi.c_str());
            return M6A_OK;
        }
        struct stat sb;
        if (fstat(f.fd, &sb) != 0) return prep_fail(M6A_EIO, "cannot stat %s", fs.c_str());
        at_site = (int64_t)sb.st_size;
        if (fstat(g.fd, &sb) != 0) return prep_fail(M6A_EIO, "cannot stat %s", fi.c_str());
        at_indiv = (int64_t)sb.st_size;
        return M6A_OK;
    }

    int close_files()
    {
        const int cf = ::close(f.fd), cg = ::close(g.fd);
        f.fd = g.fd = -1;
        if (cf != 0) return prep_fail(M6A_EIO, "cannot close %s", fs.c_str());
        if (cg != 0) return prep_fail(M6A_EIO, "cannot close %s", fi.c_str());
        return M6A_OK;
    }
};

int csv_write_impl(m6a_prep_sites &P, const char *out_dir, int write_header, int64_t n_limit, int n_threads, m6a_csv_stats &st)
{
    CsvJob<m6a_csv_stats> J(P, st);
    Rounds rd;                                              // events: start, formatted, copied
    int64_t cap = 0;
    int rc = J.begin(n_limit, n_threads, rd, 3, [&](int64_t ni, int64_t ns) { cap = std::max(cap, csv_align(ni) + ns); });
    if (rc) return rc;
    const int64_t n_rounds = J.n_rounds();
    char *dbuf[2] = {nullptr, nullptr};
    for (int i = 0; i < (n_rounds > 1 ? 2 : n_rounds ? 1 : 0); i++)
        if ((rc = J.m.alloc(dbuf[i], (size_t)cap, "CSV text")) || (rc = rd.pinned(i, cap))) return rc;
    if ((rc = J.open_files(out_dir, "", write_header, [](const char *line, int32_t n) { return std::string(line, (size_t)n); }))) return rc;

    // ---- round k + 1 is formatted and copied while round k is written
    auto queue = [&](int64_t k) -> int {
        const int i = (int)(k & 1);
        const int64_t a = J.cut[(size_t)k], b = J.cut[(size_t)k + 1], ni = J.ni(a, b);
        PCHK(hipEventRecord(rd.e[i][0], rd.s[i]));
        const int rc2 = csv_launch(J.d, J.plan, 0, a, b, dbuf[i], csv_align(ni), rd.s[i]);
        if (rc2) return rc2;
        PCHK(hipEventRecord(rd.e[i][1], rd.s[i]));
        const int64_t n = csv_align(ni) + J.ns(a, b);
        PCHK(hipMemcpyAsync(rd.pin[i], dbuf[i], (size_t)n, hipMemcpyDeviceToHost, rd.s[i]));
        g_d2h += n;
        PCHK(hipEventRecord(rd.e[i][2], rd.s[i]));
        return M6A_OK;
    };
    auto finish = [&](int64_t k) -> int {
        const int i = (int)(k & 1);
        PCHK(hipEventSynchronize(rd.e[i][2]));
        float fm = 0, cm = 0;
        PCHK(hipEventElapsedTime(&fm, rd.e[i][0], rd.e[i][1]));
        PCHK(hipEventElapsedTime(&cm, rd.e[i][1], rd.e[i][2]));
        st.ms_format += fm;
        st.ms_copy += cm;
        const int64_t a = J.cut[(size_t)k], b = J.cut[(size_t)k + 1], ni = J.ni(a, b);
        const double t0 = now_ms();
        if (!csv_pwrite_threads(J.g.fd, rd.pin[i], ni, J.at_indiv + J.plan.indiv[(size_t)a], J.nw)) return prep_fail(M6A_EIO, "cannot write %s", J.fi.c_str());
        if (!csv_pwrite_all(J.f.fd, rd.pin[i] + csv_align(ni), J.ns(a, b), J.at_site + J.plan.site[(size_t)a])) return prep_fail(M6A_EIO, "cannot write %s", J.fs.c_str());
        st.ms_write += now_ms() - t0;
        return M6A_OK;
    };
    if ((rc = run_rounds(n_rounds, queue, finish))) return rc;
    return J.close_files();
}

int csv_format_impl(int device_id, const m6a_csv_arrays &a, int64_t A, int64_t B, char *site_text, int64_t site_cap, char *indiv_text,
                    int64_t indiv_cap, int64_t *site_bytes, int64_t *indiv_bytes, int64_t *n_declined)
{
    // ---- the arrays are indexed on the device as given: every index is checked here first
    const int64_t S = a.n_sites, T = a.n_tx;
    if (S < 0 || T < 0 || a.n_rep < 1 || A < 0 || B < A || B > S) return prep_fail(M6A_EINVAL, "site range [%lld, %lld) of %lld sites", (long long)A, (long long)B, (long long)S);
    if (!a.off || !a.tx_off || (S && (!a.site_tx || !a.site_pos || !a.kmer5 || !a.site_prob || !a.mod_ratio))) return prep_fail(M6A_EINVAL, "null argument");
    if (a.off[0] != 0 || a.tx_off[0] != 0) return prep_fail(M6A_EINVAL, "offsets must start at 0");
    for (int64_t i = 0; i < S; i++) {
        if (a.off[i + 1] < a.off[i]) return prep_fail(M6A_EINVAL, "off decreases at site %lld", (long long)i);
        if ((int64_t)a.site_tx[i] >= T) return prep_fail(M6A_EINVAL, "site %lld: transcript %u of %lld", (long long)i, a.site_tx[i], (long long)T);
    }
    for (int64_t t = 0; t < T; t++)
        if (a.tx_off[t + 1] < a.tx_off[t]) return prep_fail(M6A_EINVAL, "tx_off decreases at transcript %lld", (long long)t);
    const int64_t R = a.off[S];
    if (R && (!a.read_ids || !a.read_prob || (a.n_rep > 1 && !a.read_rep))) return prep_fail(M6A_EINVAL, "null argument");
    if (T && a.tx_off[T] && !a.tx_blob) return prep_fail(M6A_EINVAL, "null argument");
    if (a.n_rep > 1)
        for (int64_t r = 0; r < R; r++)
            if (a.read_rep[r] < 0 || a.read_rep[r] >= a.n_rep) return prep_fail(M6A_EINVAL, "read %lld: replicate %d of %d", (long long)r, (int)a.read_rep[r], a.n_rep);
    if (!site_bytes || !indiv_bytes || !n_declined) return prep_fail(M6A_EINVAL, "null argument");

    DevMem m;
    int rc = open_device(device_id, m, "format fewer sites per call");
    if (rc) return rc;
    Streams st;
    PCHK(hipStreamCreateWithFlags(&st.s[0], hipStreamNonBlocking));
    hipStream_t s = st.s[0];
    int64_t *off, *tx_off, *pos;
    uint32_t *tx;
    uint8_t *k5, *blob;
    double *ids, *mr;
    int32_t *rep = nullptr;
    float *rp, *sp;
    const size_t nblob = (size_t)a.tx_off[T];
    if ((rc = m.alloc(off, (size_t)S + 1, "off")) || (rc = m.alloc(tx_off, (size_t)T + 1, "names")) || (rc = m.alloc(pos, (size_t)S, "sites")) ||
        (rc = m.alloc(tx, (size_t)S, "sites")) || (rc = m.alloc(k5, (size_t)S * 5, "sites")) || (rc = m.alloc(blob, nblob, "names")) ||
        (rc = m.alloc(ids, (size_t)R, "read ids")) || (rc = m.alloc(mr, (size_t)S, "sites")) || (rc = m.alloc(rp, (size_t)R, "reads")) ||
        (rc = m.alloc(sp, (size_t)S, "sites")) || (a.n_rep > 1 && (rc = m.alloc(rep, (size_t)R, "replicates"))))
        return rc;
    if ((rc = h2d(off, a.off, (size_t)S + 1, s)) || (rc = h2d(tx_off, a.tx_off, (size_t)T + 1, s)) || (rc = h2d(pos, a.site_pos, (size_t)S, s)) ||
        (rc = h2d(tx, a.site_tx, (size_t)S, s)) || (rc = h2d(k5, (const uint8_t *)a.kmer5, (size_t)S * 5, s)) ||
        (rc = h2d(blob, (const uint8_t *)a.tx_blob, nblob, s)) || (rc = h2d(ids, a.read_ids, (size_t)R, s)) || (rc = h2d(mr, a.mod_ratio, (size_t)S, s)) ||
        (rc = h2d(rp, a.read_prob, (size_t)R, s)) || (rc = h2d(sp, a.site_prob, (size_t)S, s)) ||
        (a.n_rep > 1 && (rc = h2d(rep, a.read_rep, (size_t)R, s))))
        return rc;
    const CsvDev d{off, tx, pos, k5, 5, 0, blob, tx_off, ids, rep, nullptr, a.n_rep, rp, sp, mr, nullptr, nullptr};
    CsvPlan plan;
    if ((rc = csv_plan(m, d, A, B, s, plan))) return rc;
    const int64_t ns = plan.site[(size_t)(B - A)], ni = plan.indiv[(size_t)(B - A)];
    *site_bytes = ns;
    *indiv_bytes = ni;
    *n_declined = plan.declined;
    if (plan.declined) return csv_declined(plan.declined);
    if (!site_text && !indiv_text) return M6A_OK;          // the sizing call
    if (!site_text || !indiv_text || site_cap < ns || indiv_cap < ni)
        return prep_fail(M6A_EINVAL, "the texts take %lld and %lld bytes, the buffers hold %lld and %lld", (long long)ns, (long long)ni,
                         (long long)site_cap, (long long)indiv_cap);
    char *out;
    if ((rc = m.alloc(out, (size_t)(csv_align(ni) + ns), "CSV text"))) return rc;
    if ((rc = csv_launch(d, plan, A, A, B, out, csv_align(ni), s))) return rc;
    if ((rc = d2h(indiv_text, out, (size_t)ni, s)) || (rc = d2h(site_text, out + csv_align(ni), (size_t)ns, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    return M6A_OK;
}

}  // namespace

extern "C" int m6a_csv_format(int device_id, const m6a_csv_arrays *a, int64_t site_begin, int64_t site_end, char *site_text, int64_t site_cap,
                              char *indiv_text, int64_t indiv_cap, int64_t *site_bytes, int64_t *indiv_bytes, int64_t *n_declined)
{
    if (!a) return prep_fail(M6A_EINVAL, "null argument");
    return guarded([&] {
        return csv_format_impl(device_id, *a, site_begin, site_end, site_text, site_cap, indiv_text, indiv_cap, site_bytes, indiv_bytes, n_declined);
    });
}

extern "C" int m6a_prep_sites_write_csv(m6a_prep_sites *p, const char *out_dir, int write_header, int64_t n_sites_limit, int n_threads,
                                        m6a_csv_stats *stats)
{
    if (!p || !out_dir) return prep_fail(M6A_EINVAL, "null argument");
    m6a_csv_stats st{};
    const int rc = guarded([&] { return csv_write_impl(*p, out_dir, write_header, n_sites_limit, n_threads, st); });
    if (stats) *stats = st;
    return rc;
}
