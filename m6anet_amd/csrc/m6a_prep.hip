// m6a_prep.hip -- `dataprep --device gpu` (include/m6a.h: m6a_prep_eventalign): eventalign.txt -> the table of runs and candidate
// rows that m6a_io_dataprep_write (include/m6a_io.h) turns into the four files.  The device restates, line for line, what the
// host's index_range, combine_read and window_rows (m6a_io.cpp) do; whatever its fast paths decline (a number with a sign or
// an exponent, more than 15 / 18 digits, a short or empty line inside a run, events out of (position, k-mer) order, a model
// k-mer that is not 5 characters) marks the run M6A_PREP_RUN_HOST and the host combines it.
//
//   upload      the file streams into HBM through two pinned staging buffers (pread into one while the other is copied);
//               nl_count_kernel counts the newlines of every 4 KB block of chunk k while chunk k + 1 is in flight
//   scan        exclusive scan of the block counts, nl_write_kernel writes every newline's offset (16-byte loads per lane)
//   lines       line_kernel, one lane per body line: the index fields (first tab, read index as atoll) and the event fields
//   runs        valid lines compacted, a run starts where the contig bytes or the read index change (index_range)
//   combine     one lane per run: Kahan sums per (position, k-mer) group, count then write
//   windows     one lane per run: runs of 2w + 1 consecutive positions with a DRACH centre, count then write
// Everything is built with -ffp-contract=off (build.py): no multiply-add is fused, and the f64 divisions are IEEE `/`.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "m6a.h"
#include "m6a_io.h"

namespace {

thread_local std::string g_prep_err;

int prep_fail(int code, const char *fmt, ...)
{
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_prep_err = buf;
    return code;
}

constexpr int kBlk = 256;                 // threads per block everywhere
constexpr int64_t kScanBytes = 4096;      // bytes per block of the newline scan: 256 lanes x 16 bytes

// per-line event flags
enum : uint8_t { L_TAB = 1, L_EMPTY = 2, L_HOST = 4, L_MATCH = 8, L_K5 = 16 };

struct LineEv {                           // one body line (line_kernel)
    int64_t position, length, kmer;       // kmer = byte offset of reference_kmer
    double mean, sd, len_s;
    int64_t read;                         // atoll of field 3
    int32_t contig_len;
    uint8_t flags;
};

struct PosRec { int64_t position, kmer; double dwell, sd, mean; };

__device__ inline int64_t line_start(const int64_t *nl, int64_t i) { return i == 0 ? 0 : nl[i - 1] + 1; }
__device__ inline int64_t line_end(const int64_t *nl, int64_t NL, int64_t n, int64_t i) { return i < NL ? nl[i] : n; }   // '\n' or EOF
__device__ inline int64_t line_next(const int64_t *nl, int64_t NL, int64_t n, int64_t i) { return i < NL ? nl[i] + 1 : n; }

// ---- newline scan ------------------------------------------------------------------------------------------------
__device__ inline int nl_in(uint32_t w)
{
    const uint32_t x = w ^ 0x0a0a0a0au;                                   // zero byte where '\n'
    const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
    return __popc(z);
}

// block b0 + blockIdx.x: its newlines, 16 bytes per lane (the buffer is padded with zeros to a whole block)
__global__ void nl_count_kernel(const uint4 *__restrict__ f, int64_t b0, int64_t *__restrict__ cnt)
{
    const int64_t b = b0 + blockIdx.x;
    const uint4 v = f[b * (kScanBytes / 16) + threadIdx.x];
    int c = nl_in(v.x) + nl_in(v.y) + nl_in(v.z) + nl_in(v.w);
    __shared__ int s[kBlk / 64];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) cnt[b] = s[0] + s[1] + s[2] + s[3];
}

__global__ void nl_write_kernel(const uint4 *__restrict__ f, int64_t nb, const int64_t *__restrict__ off, int64_t *__restrict__ nl)
{
    const int64_t b = blockIdx.x;
    if (b >= nb) return;
    const uint4 v = f[b * (kScanBytes / 16) + threadIdx.x];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    int c = 0;
    for (int k = 0; k < 4; k++) c += nl_in(w[k]);
    __shared__ int s[kBlk];
    s[threadIdx.x] = c;
    __syncthreads();
    for (int o = 1; o < kBlk; o <<= 1) {                                  // inclusive scan of the lane counts
        const int t = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    int64_t o = off[b] + s[threadIdx.x] - c;
    const int64_t at = b * kScanBytes + threadIdx.x * 16;
    for (int k = 0; k < 16; k++)
        if (((w[k >> 2] >> ((k & 3) * 8)) & 0xff) == '\n') nl[o++] = at + k;
}

// ---- exclusive scan of int64 (in place; a[n] receives the total) --------------------------------------------------
__global__ void scan_block_kernel(int64_t *__restrict__ a, int64_t n, int64_t *__restrict__ sums)
{
    const int64_t base = (int64_t)blockIdx.x * (kBlk * 4);
    int64_t v[4], t = 0;
    for (int k = 0; k < 4; k++) {
        const int64_t i = base + threadIdx.x * 4 + k;
        v[k] = i < n ? a[i] : 0;
        t += v[k];
    }
    __shared__ int64_t s[kBlk];
    s[threadIdx.x] = t;
    __syncthreads();
    for (int o = 1; o < kBlk; o <<= 1) {
        const int64_t x = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += x;
        __syncthreads();
    }
    int64_t run = s[threadIdx.x] - t;
    for (int k = 0; k < 4; k++) {
        const int64_t i = base + threadIdx.x * 4 + k;
        if (i < n) a[i] = run;
        run += v[k];
    }
    if (threadIdx.x == kBlk - 1) sums[blockIdx.x] = s[kBlk - 1];
}

__global__ void scan_add_kernel(int64_t *__restrict__ a, int64_t n, const int64_t *__restrict__ sums)
{
    const int64_t i = (int64_t)blockIdx.x * (kBlk * 4) + threadIdx.x * 4;
    const int64_t add = sums[blockIdx.x];
    for (int k = 0; k < 4; k++)
        if (i + k < n) a[i + k] += add;
}

// ---- lines ---------------------------------------------------------------------------------------------------------
__device__ inline bool dev_isspace(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

// atoll(): leading white space, a sign, digits; saturates like strtoll.  The file's end stands for the terminator.
__device__ int64_t dev_atoll(const uint8_t *f, int64_t i, int64_t n)
{
    while (i < n && dev_isspace(f[i])) ++i;
    bool neg = false;
    if (i < n && (f[i] == '+' || f[i] == '-')) { neg = f[i] == '-'; ++i; }
    const uint64_t lim = neg ? (uint64_t)1 << 63 : ((uint64_t)1 << 63) - 1;
    uint64_t v = 0;
    bool over = false;
    for (; i < n && f[i] >= '0' && f[i] <= '9'; ++i) {
        const uint64_t d = (uint64_t)(f[i] - '0');
        if (over || v > (lim - d) / 10) over = true;
        else v = v * 10 + d;
    }
    if (over) v = lim;
    return neg ? (int64_t)(0 - v) : (int64_t)v;
}

// combine_read's int_field: 1..18 plain digits
__device__ inline bool dev_int(const uint8_t *f, int64_t p, int64_t e, int64_t &out)
{
    if (p >= e || e - p > 18) return false;
    int64_t v = 0;
    for (int64_t q = p; q < e; ++q) {
        if (f[q] < '0' || f[q] > '9') return false;
        v = v * 10 + (f[q] - '0');
    }
    out = v;
    return true;
}

// combine_read's float fast path: digits [. digits], 1..15 digit characters -> mantissa / 10^frac, one IEEE division
__device__ inline bool dev_float(const uint8_t *f, int64_t p, int64_t e, double &out)
{
    const double p10[16] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};
    int64_t q = p;
    uint64_t mant = 0;
    while (q < e && (unsigned)(f[q] - '0') < 10u) mant = mant * 10 + (uint64_t)(f[q++] - '0');
    int nd = (int)(q - p), frac = 0;
    if (q < e && f[q] == '.') {
        const int64_t s = ++q;
        while (q < e && (unsigned)(f[q] - '0') < 10u) mant = mant * 10 + (uint64_t)(f[q++] - '0');
        frac = (int)(q - s);
        nd += frac;
    }
    if (q != e || nd == 0 || nd > 15) return false;
    out = (double)mant / p10[frac];
    return true;
}

// one lane per body line i = 1 .. nlines - 1 (line 0 is the header)
__global__ void line_kernel(const uint8_t *__restrict__ f, int64_t n, const int64_t *__restrict__ nl, int64_t NL, int64_t nlines,
                            LineEv *__restrict__ ev, unsigned long long *__restrict__ bad_at)
{
    const int64_t i = 1 + (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= nlines) return;
    const int64_t p = line_start(nl, i), le = line_end(nl, NL, n, i);
    LineEv r;
    r.flags = 0; r.position = r.length = r.kmer = r.read = 0; r.mean = r.sd = r.len_s = 0; r.contig_len = 0;
    int64_t fe[16];
    int nf = 0, ntab = 0;
    for (int64_t q = p; q < le; ++q)
        if (f[q] == '\t') { if (nf < 16) fe[nf++] = q; ++ntab; }
    if (nf < 16) fe[nf++] = le;
    // index_range: no tab -> skipped; fewer than three -> M6A_IO_EFORMAT at the line's offset
    if (ntab >= 1) {
        r.flags |= L_TAB;
        if (ntab < 3) atomicMin(bad_at, (unsigned long long)p);
        else r.read = dev_atoll(f, fe[2] + 1, n);
        r.contig_len = (int32_t)min<int64_t>(fe[0] - p, 0x7fffffff);
        if (fe[0] - p > 0x7fffffff) r.flags |= L_HOST;
    }
    // combine_read
    int64_t eol = le;
    if (eol > p && f[eol - 1] == '\r') --eol;
    if (eol == p) r.flags |= L_EMPTY;
    else if (nf < 15) r.flags |= L_HOST;                  // malformed: the host reports it if the run is reached
    else {
        if (fe[nf - 1] > eol) fe[nf - 1] = eol;
        const int64_t b2 = fe[1] + 1, b9 = fe[8] + 1, len = fe[2] - b2;
        bool match = len == fe[9] - b9;
        for (int64_t k = 0; match && k < len; k++) match = f[b2 + k] == f[b9 + k];
        if (match) {
            r.flags |= L_MATCH;
            if (len == 5) r.flags |= L_K5;
            r.kmer = b2;
            int64_t st, ed;
            if (!dev_int(f, fe[0] + 1, fe[1], r.position) || !dev_float(f, fe[5] + 1, fe[6], r.mean) || !dev_float(f, fe[6] + 1, fe[7], r.sd) ||
                !dev_float(f, fe[7] + 1, fe[8], r.len_s) || !dev_int(f, fe[12] + 1, fe[13], st) || !dev_int(f, fe[13] + 1, fe[14], ed))
                r.flags |= L_HOST;
            else r.length = ed - st;
        }
    }
    ev[i] = r;
}

__global__ void flag_kernel(const LineEv *__restrict__ ev, int64_t nlines, int64_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i < nlines) out[i] = i >= 1 && (ev[i].flags & L_TAB) ? 1 : 0;
}

__global__ void compact_kernel(const int64_t *__restrict__ flag_scan, int64_t nlines, const LineEv *__restrict__ ev, int64_t *__restrict__ vline)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= 1 && i < nlines && (ev[i].flags & L_TAB)) vline[flag_scan[i]] = i;
}

__device__ inline bool same_bytes(const uint8_t *f, int64_t a, int64_t b, int64_t len)
{
    for (int64_t k = 0; k < len; k++)
        if (f[a + k] != f[b + k]) return false;
    return true;
}

// valid line j starts a run when its contig bytes or its read index differ from valid line j - 1's
__global__ void newrun_kernel(const uint8_t *__restrict__ f, const int64_t *__restrict__ nl, const LineEv *__restrict__ ev,
                              const int64_t *__restrict__ vline, int64_t NV, int64_t *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (j >= NV) return;
    if (j == 0) { out[0] = 1; return; }
    const int64_t a = vline[j - 1], b = vline[j];
    const LineEv &x = ev[a], &y = ev[b];
    out[j] = x.read != y.read || x.contig_len != y.contig_len || !same_bytes(f, line_start(nl, a), line_start(nl, b), y.contig_len) ? 1 : 0;
}

struct RunDev {                            // one run: lines [l0, l1], bytes [start, end)
    int64_t l0, l1, start, end, read, contig, npos;
    int32_t contig_len, status, same_contig;
};

__global__ void runs_kernel(const uint8_t *__restrict__ f, int64_t n, const int64_t *__restrict__ nl, int64_t NL, const LineEv *__restrict__ ev,
                            const int64_t *__restrict__ vline, int64_t NV, const int64_t *__restrict__ nr_scan, RunDev *__restrict__ runs)
{
    const int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (j >= NV) return;
    const int64_t r = nr_scan[j] - 1;                   // inclusive count of run starts up to j
    const bool first = j == 0 || nr_scan[j - 1] != nr_scan[j];
    const bool last = j == NV - 1 || nr_scan[j + 1] != nr_scan[j];
    const int64_t li = vline[j];
    if (first) {
        RunDev &R = runs[r];
        R.l0 = li;
        R.start = line_start(nl, li);
        R.read = ev[li].read;
        R.contig = R.start;
        R.contig_len = ev[li].contig_len;
        R.status = M6A_PREP_RUN_OK;
        R.npos = 0;
        R.same_contig = 0;
        if (r > 0) {                                       // same contig bytes as the run before (transcript ids on the host)
            const int64_t pl = vline[j - 1];
            R.same_contig = ev[pl].contig_len == ev[li].contig_len && same_bytes(f, line_start(nl, pl), R.start, ev[li].contig_len);
        }
    }
    if (last) {
        runs[r].l1 = li;
        runs[r].end = line_next(nl, NL, n, li);
    }
}

// --skip_index: the lines of every run's byte range [start, end), or M6A_PREP_RUN_HOST where the range is not whole body lines
__global__ void runs_from_index_kernel(int64_t n, const int64_t *__restrict__ nl, int64_t NL, int64_t nlines, RunDev *__restrict__ runs, int64_t NR)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r >= NR) return;
    RunDev &R = runs[r];
    R.npos = 0;
    R.status = M6A_PREP_RUN_HOST;
    if (R.start < 0 || R.end > n || R.start >= R.end) return;
    // first line whose start >= R.start: line i starts at nl[i - 1] + 1
    int64_t lo = 0, hi = NL;                               // search nl for the first newline >= R.start - 1
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (nl[m] + 1 < R.start) lo = m + 1; else hi = m; }
    const int64_t l0 = lo + 1;                             // nl[lo] + 1 >= R.start
    if (lo >= NL || nl[lo] + 1 != R.start || l0 >= nlines) return;
    // last line whose next == R.end
    lo = 0; hi = NL;
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (nl[m] + 1 < R.end) lo = m + 1; else hi = m; }
    int64_t l1;
    if (lo < NL && nl[lo] + 1 == R.end) l1 = lo;
    else if (R.end == n && nlines > NL) l1 = nlines - 1;   // the last line, without its newline
    else return;
    if (l1 < l0) return;
    R.l0 = l0; R.l1 = l1;
    R.status = M6A_PREP_RUN_OK;
}

__device__ inline int kcmp5(const uint8_t *f, int64_t a, int64_t b)
{
    for (int k = 0; k < 5; k++)
        if (f[a + k] != f[b + k]) return f[a + k] < f[b + k] ? -1 : 1;
    return 0;
}

// combine_read over lines [l0, l1]: count (out == nullptr) or write the per-(position, k-mer) means
__global__ void combine_kernel(const uint8_t *__restrict__ f, const LineEv *__restrict__ ev, RunDev *__restrict__ runs, int64_t NR,
                               const int64_t *__restrict__ pos_off, PosRec *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r >= NR) return;
    RunDev &R = runs[r];
    if (R.status != M6A_PREP_RUN_OK) return;
    int64_t np = 0, o = out ? pos_off[r] : 0;
    bool have = false;
    int64_t gpos = 0, gk = 0, total = 0;
    double s_sum = 0, s_comp = 0, d_sum = 0, d_comp = 0, m_sum = 0, m_comp = 0;
    auto kadd = [](double &sum, double &comp, double v) {
        const double y = v - comp, t = sum + y;
        comp = t - sum - y;
        if (comp != comp) comp = 0;
        sum = t;
    };
    auto flush = [&]() {
        if (out) {
            PosRec p;
            p.position = gpos; p.kmer = gk;
            p.mean = rint(m_sum / (double)total * 10.0) / 10.0;
            p.sd = s_sum / (double)total;
            p.dwell = d_sum / (double)total;
            out[o++] = p;
        }
        ++np;
    };
    for (int64_t li = R.l0; li <= R.l1; ++li) {
        const LineEv &e = ev[li];
        if (!(e.flags & L_TAB) || (e.flags & L_HOST)) { if (!out) R.status = M6A_PREP_RUN_HOST; return; }
        if (!(e.flags & L_MATCH)) continue;
        if (!(e.flags & L_K5)) { if (!out) R.status = M6A_PREP_RUN_HOST; return; }
        if (have) {
            const int c = kcmp5(f, gk, e.kmer);
            if (gpos > e.position || (gpos == e.position && c > 0)) { if (!out) R.status = M6A_PREP_RUN_HOST; return; }
            if (gpos != e.position || c != 0) { flush(); have = false; }
        }
        if (!have) {
            have = true; gpos = e.position; gk = e.kmer; total = 0;
            s_sum = s_comp = d_sum = d_comp = m_sum = m_comp = 0;
        }
        const double len = (double)e.length;
        kadd(m_sum, m_comp, e.mean * len);
        kadd(s_sum, s_comp, e.sd * len);
        kadd(d_sum, d_comp, e.len_s * len);
        total += e.length;
    }
    if (have) flush();
    if (!out) R.npos = np;
}

__device__ inline bool dev_drach(const uint8_t *k)
{
    return (k[0] == 'A' || k[0] == 'G' || k[0] == 'T') && (k[1] == 'G' || k[1] == 'A') && k[2] == 'A' && k[3] == 'C' &&
           (k[4] == 'A' || k[4] == 'C' || k[4] == 'T');
}

// window_rows over one run's combined positions: count (row_pos == nullptr) or write the candidate rows
__global__ void window_kernel(const uint8_t *__restrict__ f, const RunDev *__restrict__ runs, int64_t NR, const int64_t *__restrict__ pos_off,
                              const PosRec *__restrict__ ps, int w, int64_t *__restrict__ row_cnt, const int64_t *__restrict__ row_off,
                              int64_t *__restrict__ row_pos, uint8_t *__restrict__ row_kmer, double *__restrict__ row_feat)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r >= NR) return;
    const RunDev &R = runs[r];
    if (R.status != M6A_PREP_RUN_OK) { if (!row_pos) row_cnt[r] = 0; return; }
    const PosRec *p = ps + pos_off[r];
    const int64_t np = R.npos, K = 5 + 2 * w, NF = 3 * (2 * w + 1);
    int64_t run = 0, nrow = 0, o = row_pos ? row_off[r] : 0;
    for (int64_t i = 0; i < np; i++) {
        run = i > 0 && p[i].position == p[i - 1].position + 1 ? run + 1 : 1;
        if (run < 2 * w + 1) continue;
        const int64_t c = i - w;                           // the window [c - w, c + w] is consecutive
        if (!dev_drach(f + p[c].kmer)) continue;
        if (row_pos) {
            row_pos[o] = p[c].position + 2;
            uint8_t *km = row_kmer + o * K;
            for (int k = 0; k < 5; k++) km[k] = f[p[c - w].kmer + k];
            for (int64_t k = c - w + 1; k <= c + w; k++) km[5 + (k - (c - w + 1))] = f[p[k].kmer + 4];
            double *ft = row_feat + o * NF;
            for (int64_t k = c - w; k <= c + w; k++) {
                *ft++ = p[k].dwell; *ft++ = p[k].sd; *ft++ = p[k].mean;
            }
            ++o;
        }
        ++nrow;
    }
    if (!row_pos) row_cnt[r] = nrow;
}

__global__ void run_cols_kernel(const RunDev *__restrict__ runs, int64_t NR, int64_t *__restrict__ npos)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r < NR) npos[r] = runs[r].status == M6A_PREP_RUN_OK ? runs[r].npos : 0;
}

inline unsigned grid(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + kBlk - 1) / kBlk); }

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

// ---- the handle ----------------------------------------------------------------------------------------------------
struct m6a_prep {
    m6a_io_prep_table t{};
    std::string blob;
    std::vector<int64_t> tx_off, run_read, run_start, run_end, run_npos, row_off, row_pos;
    std::vector<uint32_t> run_tx;
    std::vector<int32_t> run_status;
    std::vector<char> kmer;
    std::vector<double> feat;
    double ms[6] = {0, 0, 0, 0, 0, 0};     // upload (+ newline count), newline offsets, lines + runs + combine + windows, D2H, host, H2D GB/s
};

namespace {

#define PCHK(x)                                                                                                            \
    do {                                                                                                                   \
        hipError_t e_ = (x);                                                                                               \
        if (e_ != hipSuccess) return prep_fail(M6A_EHIP, "%s: %s", #x, hipGetErrorString(e_));                             \
    } while (0)

// device memory of one call, every allocation counted against the budget (free memory minus a margin, or M6A_PREP_BUDGET_MB)
struct DevMem {
    std::vector<void *> ptrs;
    size_t used = 0, budget = 0;
    ~DevMem() { for (void *p : ptrs) (void)hipFree(p); }
    template <class T> int alloc(T *&p, size_t count, const char *what)
    {
        const size_t bytes = std::max<size_t>(16, count * sizeof(T));
        if (used + bytes > budget)
            return prep_fail(M6A_ENOMEM, "dataprep on the device needs more than its budget of %zu MB (%s: %zu MB used, %zu MB more); "
                             "this file does not fit: use --device cpu", budget >> 20, what, used >> 20, bytes >> 20);
        void *q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) return prep_fail(M6A_ENOMEM, "hipMalloc of %zu MB failed (%s); use --device cpu", bytes >> 20, what);
        ptrs.push_back(q);
        used += bytes;
        p = (T *)q;
        return M6A_OK;
    }
};

struct Streams {
    hipStream_t s[2] = {nullptr, nullptr};
    hipEvent_t copied[2] = {nullptr, nullptr};
    void *pin[2] = {nullptr, nullptr};
    ~Streams()
    {
        for (int i = 0; i < 2; i++) {
            if (s[i]) (void)hipStreamSynchronize(s[i]);
        }
        for (int i = 0; i < 2; i++) {
            if (copied[i]) (void)hipEventDestroy(copied[i]);
            if (pin[i]) (void)hipHostFree(pin[i]);
            if (s[i]) (void)hipStreamDestroy(s[i]);
        }
    }
};

struct Fd {
    int fd = -1;
    ~Fd() { if (fd >= 0) ::close(fd); }
};

int scan_excl(DevMem &m, int64_t *a, int64_t n, hipStream_t s)
{
    const int64_t per = kBlk * 4, nb = (n + per - 1) / per;
    if (n <= 0) return M6A_OK;
    int64_t *sums;
    int rc = m.alloc(sums, (size_t)nb + 1, "scan");
    if (rc) return rc;
    scan_block_kernel<<<(unsigned)nb, kBlk, 0, s>>>(a, n, sums);
    PCHK(hipGetLastError());
    if (nb > 1) {
        if ((rc = scan_excl(m, sums, nb, s))) return rc;
        scan_add_kernel<<<(unsigned)nb, kBlk, 0, s>>>(a, n, sums);
        PCHK(hipGetLastError());
    }
    return M6A_OK;
}

// a[n] = sum of a[0..n) after the scan: the array holds n + 1 elements, the last one 0 before it
int scan_total(DevMem &m, int64_t *a, int64_t n, hipStream_t s, int64_t &total)
{
    PCHK(hipMemsetAsync(a + n, 0, sizeof(int64_t), s));
    int rc = scan_excl(m, a, n + 1, s);
    if (rc) return rc;
    PCHK(hipMemcpyAsync(&total, a + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    PCHK(hipStreamSynchronize(s));
    return M6A_OK;
}

// the rows of an existing eventalign.index, as m6a_io.cpp's read_index_file reads them
int read_index(const char *path, std::vector<std::string> &names, std::vector<uint32_t> &tx, std::vector<int64_t> &read,
               std::vector<int64_t> &start, std::vector<int64_t> &end)
{
    FILE *f = fopen(path, "r");
    if (!f) return prep_fail(M6A_EIO, "--skip_index but %s does not exist", path);
    std::unordered_map<std::string, uint32_t> ids;
    char line[4096];
    bool first = true;
    while (fgets(line, sizeof line, f)) {
        if (first) { first = false; continue; }
        char *c = strrchr(line, ',');
        if (!c) continue;
        const int64_t e = atoll(c + 1); *c = 0;
        c = strrchr(line, ','); if (!c) continue;
        const int64_t s = atoll(c + 1); *c = 0;
        c = strrchr(line, ','); if (!c) continue;
        const int64_t r = atoll(c + 1); *c = 0;
        const size_t n = strlen(line);
        uint32_t id;
        if (!tx.empty() && names[tx.back()].size() == n && memcmp(names[tx.back()].data(), line, n) == 0) id = tx.back();
        else {
            auto it = ids.find(std::string(line, n));
            if (it != ids.end()) id = it->second;
            else { id = (uint32_t)names.size(); ids.emplace(std::string(line, n), id); names.emplace_back(line, n); }
        }
        tx.push_back(id); read.push_back(r); start.push_back(s); end.push_back(e);
    }
    fclose(f);
    return M6A_OK;
}

int prep_impl(int device_id, const char *path, int w, const char *index_path, m6a_prep &P)
{
    if (w < 1 || w > 16) return prep_fail(M6A_EINVAL, "n_neighbors must be 1..16");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return prep_fail(M6A_ENODEV, "no HIP device");
    if (device_id < 0 || device_id >= ndev) return prep_fail(M6A_EINVAL, "device %d of %d", device_id, ndev);
    PCHK(hipSetDevice(device_id));
    Fd fd;
    fd.fd = ::open(path, O_RDONLY);
    if (fd.fd < 0) return prep_fail(M6A_EIO, "cannot open %s", path);
    struct stat st;
    if (fstat(fd.fd, &st) != 0) return prep_fail(M6A_EIO, "cannot stat %s", path);
    const int64_t n = (int64_t)st.st_size;

    // --skip_index: the runs come from the file (read before anything touches the device, as the host path does)
    std::vector<std::string> names;
    std::vector<uint32_t> itx;
    std::vector<int64_t> iread, istart, iend;
    if (index_path) {
        int rc = read_index(index_path, names, itx, iread, istart, iend);
        if (rc) return rc;
    }

    DevMem m;
    {
        size_t fr = 0, tot = 0;
        PCHK(hipMemGetInfo(&fr, &tot));
        const size_t margin = std::min<size_t>(fr / 16, (size_t)4 << 30);
        m.budget = fr > margin ? fr - margin : 0;
        const char *b = getenv("M6A_PREP_BUDGET_MB");
        if (b && atoll(b) > 0) m.budget = std::min(m.budget, (size_t)atoll(b) << 20);
    }
    const int64_t nb = std::max<int64_t>(1, (n + kScanBytes - 1) / kScanBytes);       // 4 KB scan blocks; the buffer is padded to them
    uint8_t *df;
    int64_t *bcnt;
    int rc = m.alloc(df, (size_t)(nb * kScanBytes), "the file");
    if (!rc) rc = m.alloc(bcnt, (size_t)nb + 1, "newline counts");
    if (rc) return rc;

    Streams S;
    for (int i = 0; i < 2; i++) {
        PCHK(hipStreamCreateWithFlags(&S.s[i], hipStreamNonBlocking));
        PCHK(hipEventCreateWithFlags(&S.copied[i], hipEventDisableTiming));
    }
    hipStream_t s = S.s[0];                                  // kernels; S.s[1] copies
    const char *ck = getenv("M6A_PREP_CHUNK_KB");
    int64_t chunk = (ck && atoll(ck) > 0 ? atoll(ck) : 65536) << 10;
    chunk = std::max<int64_t>(kScanBytes, (chunk + kScanBytes - 1) / kScanBytes * kScanBytes);
    chunk = std::min<int64_t>(chunk, nb * kScanBytes);
    for (int i = 0; i < 2; i++) PCHK(hipHostMalloc(&S.pin[i], (size_t)chunk, hipHostMallocDefault));
    PCHK(hipMemsetAsync(df + (nb - 1) * kScanBytes, 0, (size_t)kScanBytes, S.s[1]));        // the zero padding of the last block

    // ---- upload: pread chunk k into one pinned buffer while chunk k - 1 is copied and counted
    const double t_up = now_ms();
    for (int64_t k = 0, off = 0; off < n; k++, off += chunk) {
        const int slot = (int)(k & 1);
        PCHK(hipEventSynchronize(S.copied[slot]));          // the copy that last used this buffer is done
        const int64_t len = std::min(chunk, n - off);
        for (int64_t got = 0; got < len;) {
            const ssize_t r = ::pread(fd.fd, (char *)S.pin[slot] + got, (size_t)(len - got), (off_t)(off + got));
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) return prep_fail(M6A_EIO, "cannot read %s", path);
            got += r;
        }
        PCHK(hipMemcpyAsync(df + off, S.pin[slot], (size_t)len, hipMemcpyHostToDevice, S.s[1]));
        PCHK(hipEventRecord(S.copied[slot], S.s[1]));
        PCHK(hipStreamWaitEvent(s, S.copied[slot], 0));
        const int64_t b0 = off / kScanBytes, b1 = std::min(nb, (off + len + kScanBytes - 1) / kScanBytes);
        nl_count_kernel<<<(unsigned)(b1 - b0), kBlk, 0, s>>>((const uint4 *)df, b0, bcnt);
        PCHK(hipGetLastError());
    }
    if (n == 0) PCHK(hipMemsetAsync(bcnt, 0, sizeof(int64_t), s));
    PCHK(hipStreamSynchronize(S.s[1]));
    PCHK(hipStreamSynchronize(s));
    P.ms[0] = now_ms() - t_up;
    P.ms[5] = P.ms[0] > 0 ? (double)n / (P.ms[0] * 1e6) : 0;

    // ---- newline offsets
    double t1 = now_ms();
    int64_t NL = 0;
    if ((rc = scan_total(m, bcnt, nb, s, NL))) return rc;
    if (!index_path && NL == 0) return prep_fail(M6A_EFORMAT, "%s: no header line", path);
    int64_t *nl;
    if ((rc = m.alloc(nl, (size_t)NL + 1, "newline offsets"))) return rc;
    nl_write_kernel<<<(unsigned)nb, kBlk, 0, s>>>((const uint4 *)df, nb, bcnt, nl);
    PCHK(hipGetLastError());
    uint8_t last = '\n';
    if (n > 0) PCHK(hipMemcpyAsync(&last, df + n - 1, 1, hipMemcpyDeviceToHost, s));
    PCHK(hipStreamSynchronize(s));
    const int64_t nlines = NL + (last != '\n' ? 1 : 0);
    P.ms[1] = now_ms() - t1;

    // ---- lines, runs, combine, windows
    t1 = now_ms();
    LineEv *ev;
    unsigned long long *bad;
    if ((rc = m.alloc(ev, (size_t)std::max<int64_t>(nlines, 1), "line records"))) return rc;
    if ((rc = m.alloc(bad, 1, "flags"))) return rc;
    const unsigned long long none = ~0ull;
    PCHK(hipMemcpyAsync(bad, &none, sizeof none, hipMemcpyHostToDevice, s));
    if (nlines > 1) {
        line_kernel<<<grid(nlines - 1), kBlk, 0, s>>>(df, n, nl, NL, nlines, ev, bad);
        PCHK(hipGetLastError());
    }
    unsigned long long bad_at = none;
    PCHK(hipMemcpyAsync(&bad_at, bad, sizeof bad_at, hipMemcpyDeviceToHost, s));
    PCHK(hipStreamSynchronize(s));
    if (!index_path && bad_at != none) return prep_fail(M6A_EFORMAT, "%s: short line at byte %lld", path, (long long)bad_at);

    int64_t NR = 0;
    RunDev *runs = nullptr;
    if (!index_path) {
        int64_t *vflag, NV = 0;
        if ((rc = m.alloc(vflag, (size_t)nlines + 1, "valid lines"))) return rc;
        flag_kernel<<<grid(nlines), kBlk, 0, s>>>(ev, nlines, vflag);
        PCHK(hipGetLastError());
        if ((rc = scan_total(m, vflag, nlines, s, NV))) return rc;
        int64_t *vline, *nr;
        if ((rc = m.alloc(vline, (size_t)NV + 1, "valid lines"))) return rc;
        if ((rc = m.alloc(nr, (size_t)NV + 1, "run starts"))) return rc;
        compact_kernel<<<grid(nlines), kBlk, 0, s>>>(vflag, nlines, ev, vline);
        PCHK(hipGetLastError());
        if (NV > 0) {
            newrun_kernel<<<grid(NV), kBlk, 0, s>>>(df, nl, ev, vline, NV, nr);
            PCHK(hipGetLastError());
        }
        if ((rc = scan_total(m, nr, NV, s, NR))) return rc;     // nr[j] = run of valid line j (exclusive scan of the starts) ...
        // ... so valid line j's run is nr[j + 1] - 1: shift by one with an inclusive view
        if ((rc = m.alloc(runs, (size_t)NR + 1, "runs"))) return rc;
        if (NV > 0) {
            runs_kernel<<<grid(NV), kBlk, 0, s>>>(df, n, nl, NL, ev, vline, NV, nr + 1, runs);
            PCHK(hipGetLastError());
        }
    } else {
        NR = (int64_t)istart.size();
        if ((rc = m.alloc(runs, (size_t)NR + 1, "runs"))) return rc;
        std::vector<RunDev> h((size_t)NR);
        for (int64_t r = 0; r < NR; r++) { h[(size_t)r].start = istart[(size_t)r]; h[(size_t)r].end = iend[(size_t)r]; }
        if (NR) PCHK(hipMemcpyAsync(runs, h.data(), (size_t)NR * sizeof(RunDev), hipMemcpyHostToDevice, s));
        if (NR) {
            runs_from_index_kernel<<<grid(NR), kBlk, 0, s>>>(n, nl, NL, nlines, runs, NR);
            PCHK(hipGetLastError());
        }
        PCHK(hipStreamSynchronize(s));                        // h goes out of scope
    }
    int64_t *pos_off, NP = 0;
    if ((rc = m.alloc(pos_off, (size_t)NR + 1, "positions"))) return rc;
    if (NR) {
        combine_kernel<<<grid(NR), kBlk, 0, s>>>(df, ev, runs, NR, nullptr, nullptr);
        PCHK(hipGetLastError());
        run_cols_kernel<<<grid(NR), kBlk, 0, s>>>(runs, NR, pos_off);
        PCHK(hipGetLastError());
    }
    if ((rc = scan_total(m, pos_off, NR, s, NP))) return rc;
    PosRec *ps;
    if ((rc = m.alloc(ps, (size_t)NP + 1, "combined positions"))) return rc;
    int64_t *row_off, NROW = 0;
    if ((rc = m.alloc(row_off, (size_t)NR + 1, "rows"))) return rc;
    if (NR) {
        combine_kernel<<<grid(NR), kBlk, 0, s>>>(df, ev, runs, NR, pos_off, ps);
        PCHK(hipGetLastError());
        window_kernel<<<grid(NR), kBlk, 0, s>>>(df, runs, NR, pos_off, ps, w, row_off, nullptr, nullptr, nullptr, nullptr);
        PCHK(hipGetLastError());
    }
    if ((rc = scan_total(m, row_off, NR, s, NROW))) return rc;
    const int64_t K = 5 + 2 * w, NF = 3 * (2 * w + 1);
    int64_t *drow_pos;
    uint8_t *drow_kmer;
    double *drow_feat;
    if ((rc = m.alloc(drow_pos, (size_t)NROW, "rows"))) return rc;
    if ((rc = m.alloc(drow_kmer, (size_t)(NROW * K), "rows"))) return rc;
    if ((rc = m.alloc(drow_feat, (size_t)(NROW * NF), "rows"))) return rc;
    if (NR && NROW) {
        window_kernel<<<grid(NR), kBlk, 0, s>>>(df, runs, NR, pos_off, ps, w, nullptr, row_off, drow_pos, drow_kmer, drow_feat);
        PCHK(hipGetLastError());
    }
    PCHK(hipStreamSynchronize(s));
    P.ms[2] = now_ms() - t1;

    // ---- to the host
    t1 = now_ms();
    std::vector<RunDev> hr((size_t)NR);
    P.row_off.resize((size_t)NR + 1);
    P.row_pos.resize((size_t)NROW);
    P.kmer.resize((size_t)(NROW * K));
    P.feat.resize((size_t)(NROW * NF));
    if (NR) PCHK(hipMemcpyAsync(hr.data(), runs, (size_t)NR * sizeof(RunDev), hipMemcpyDeviceToHost, s));
    PCHK(hipMemcpyAsync(P.row_off.data(), row_off, (size_t)(NR + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (NROW) {
        PCHK(hipMemcpyAsync(P.row_pos.data(), drow_pos, (size_t)NROW * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        PCHK(hipMemcpyAsync(P.kmer.data(), drow_kmer, (size_t)(NROW * K), hipMemcpyDeviceToHost, s));
        PCHK(hipMemcpyAsync(P.feat.data(), drow_feat, (size_t)(NROW * NF) * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    PCHK(hipStreamSynchronize(s));
    P.ms[3] = now_ms() - t1;

    // ---- the run table; contig names interned in order of first appearance (read from the file where the contig changes)
    t1 = now_ms();
    P.run_tx.resize((size_t)NR); P.run_read.resize((size_t)NR); P.run_start.resize((size_t)NR); P.run_end.resize((size_t)NR);
    P.run_npos.resize((size_t)NR); P.run_status.resize((size_t)NR);
    if (index_path) {
        for (const std::string &nm : names) { P.tx_off.push_back((int64_t)P.blob.size()); P.blob += nm; }
        P.tx_off.push_back((int64_t)P.blob.size());
        P.run_tx = itx; P.run_read = iread; P.run_start = istart; P.run_end = iend;
    } else {
        std::unordered_map<std::string, uint32_t> ids;
        std::string nm;
        uint32_t cur = 0;
        for (int64_t r = 0; r < NR; r++) {
            const RunDev &R = hr[(size_t)r];
            if (r == 0 || !R.same_contig) {
                nm.resize((size_t)R.contig_len);
                for (int64_t got = 0; got < R.contig_len;) {
                    const ssize_t k = ::pread(fd.fd, &nm[(size_t)got], (size_t)(R.contig_len - got), (off_t)(R.contig + got));
                    if (k < 0 && errno == EINTR) continue;
                    if (k <= 0) return prep_fail(M6A_EIO, "cannot read %s", path);
                    got += k;
                }
                auto it = ids.find(nm);
                if (it != ids.end()) cur = it->second;
                else {
                    cur = (uint32_t)ids.size();
                    ids.emplace(nm, cur);
                    P.tx_off.push_back((int64_t)P.blob.size());
                    P.blob += nm;
                }
            }
            P.run_tx[(size_t)r] = cur;
            P.run_read[(size_t)r] = R.read;
            P.run_start[(size_t)r] = R.start;
            P.run_end[(size_t)r] = R.end;
        }
        P.tx_off.push_back((int64_t)P.blob.size());
    }
    for (int64_t r = 0; r < NR; r++) {
        P.run_status[(size_t)r] = hr[(size_t)r].status;
        P.run_npos[(size_t)r] = hr[(size_t)r].status == M6A_PREP_RUN_OK ? hr[(size_t)r].npos : 0;
    }
    m6a_io_prep_table &t = P.t;
    t.n_neighbors = w;
    t.n_tx = (int64_t)P.tx_off.size() - 1; t.tx_blob = P.blob.data(); t.tx_off = P.tx_off.data();
    t.n_runs = NR; t.run_tx = P.run_tx.data(); t.run_read = P.run_read.data(); t.run_start = P.run_start.data(); t.run_end = P.run_end.data();
    t.run_npos = P.run_npos.data(); t.run_status = P.run_status.data(); t.row_off = P.row_off.data();
    t.n_rows = NROW; t.row_pos = P.row_pos.data(); t.row_kmer = P.kmer.data(); t.row_feat = P.feat.data();
    P.ms[4] = now_ms() - t1;
    return M6A_OK;
}

}  // namespace

extern "C" int m6a_prep_eventalign(int device_id, const char *path, int n_neighbors, const char *index_path, m6a_prep **out)
{
    if (!path || !out) return prep_fail(M6A_EINVAL, "null argument");
    *out = nullptr;
    m6a_prep *p = new (std::nothrow) m6a_prep;
    if (!p) return prep_fail(M6A_ENOMEM, "out of host memory");
    int rc;
    try {
        rc = prep_impl(device_id, path, n_neighbors, index_path, *p);
    } catch (const std::bad_alloc &) {
        rc = prep_fail(M6A_ENOMEM, "out of host memory");
    } catch (...) {
        rc = prep_fail(M6A_EIO, "unexpected exception");
    }
    if (rc) { delete p; return rc; }
    *out = p;
    return M6A_OK;
}

extern "C" const m6a_io_prep_table *m6a_prep_table(const m6a_prep *p) { return p ? &p->t : nullptr; }
extern "C" int m6a_prep_times(const m6a_prep *p, double *ms6)
{
    if (!p || !ms6) return prep_fail(M6A_EINVAL, "null argument");
    for (int i = 0; i < 6; i++) ms6[i] = p->ms[i];
    return M6A_OK;
}
extern "C" void m6a_prep_free(m6a_prep *p) { delete p; }
extern "C" const char *m6a_prep_last_error(void) { return g_prep_err.c_str(); }
