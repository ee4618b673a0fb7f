// m6a_prep.hip -- `dataprep --device gpu` (include/m6a.h: m6a_prep_eventalign): eventalign.txt -> the table of runs and candidate
// rows that m6a_io_dataprep_write (include/m6a_io.h) turns into the four files.  The device restates, line for line, what the
// host's index_range, combine_read and window_rows (m6a_io.cpp) do; whatever its fast paths decline marks the run
// M6A_PREP_RUN_HOST and the host combines it.  A run is declined exactly when (tests/eventalign_statement.py: declines)
//   - one of its lines has no tab (an empty line, too) or fewer than 15 fields, or its contig name is longer than an int32 holds;
//   - on a line whose reference_kmer equals model_kmer: a float field that is not digits [. digits] with 1..15 digit characters
//     (a sign, an exponent, a name, 16 digits), position / start_idx / end_idx that is not 1..18 plain digits, or a k-mer that
//     is not 5 characters -- the fields of lines whose k-mers differ are never read, so nothing in them declines a run;
//   - two such lines follow each other out of (position, k-mer) order;
//   - with --skip_index, its byte range is not whole body lines.
//
//   upload      the file streams into HBM through two pinned staging buffers (pread into one while the other is copied);
//               nl_count_kernel counts the newlines of every 4 KB block of chunk k while chunk k + 1 is in flight
//   scan        exclusive scan of the block counts, nl_write_kernel writes every newline's offset (16-byte loads per lane)
//   lines       line_kernel, one lane per body line: the index fields (first tab, read index as atoll) and the event fields
//   runs        valid lines compacted, a run starts where the contig bytes or the read index change (index_range)
//   combine     one lane per run: Kahan sums per (position, k-mer) group, count then write
//   windows     one lane per run: runs of 2w + 1 consecutive positions with a DRACH centre, count then write
// With a window size (M6A_PREP_WINDOW_KB, m6a_prep_sites_build_windows) the same kernels run on one window of the file after the other
// and only runs and rows stay on the device: front_windows, below, over a FileSource.  Text from a pipe (`-`, a FIFO) goes through the
// same windows as it arrives, and what the back half would read again is saved from every window: the same loop over a StreamSource.
// Input grouped by transcript (m6a_prep_group) stops that loop between two windows: the back half runs on the transcripts that are
// complete, their runs and rows leave the device, and the sites come out in batches cut on flush boundaries.
// Everything is built with -ffp-contract=off (build.py): no multiply-add is fused, and the f64 divisions are IEEE `/`.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "m6a.h"
#include "m6a_io.h"
#include "m6a_prep_kit.h"
#include "m6a_stream.h"
#include "m6a_uuid.h"

namespace {

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

using Name = m6a_uuid::Name;                // a read name (--read_names): 128 bits, kept beside the line and run records, never in them

// one lane per body line i = first .. nlines - 1 (first = 1: line 0 is the header; 0 in a window behind the first, which has none).
// NAMES (m6a_prep_sites_build_names): field 4 is a read name, parsed by m6a_uuid.h into lname[i]; `read` stays 0 until the names
// are interned.  bad_at is then twice the offset, plus 1 for a name that is no UUID (its field's offset) and 0 for a short line
// (its line's): one atomicMin finds the lowest of either kind.
template <bool NAMES>
__global__ void line_kernel(const uint8_t *__restrict__ f, int64_t n, const int64_t *__restrict__ nl, int64_t NL, int64_t nlines, int64_t first,
                            LineEv *__restrict__ ev, unsigned long long *__restrict__ bad_at, Name *__restrict__ lname)
{
    const int64_t i = first + (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= nlines) return;
    const int64_t p = line_start(nl, i), le = line_end(nl, NL, n, i);
    LineEv r;
    r.flags = 0; r.position = r.length = r.kmer = r.read = 0; r.mean = r.sd = r.len_s = 0; r.contig_len = 0;
    Name nm{0, 0};
    int64_t fe[16];
    int nf = 0, ntab = 0;
    for (int64_t q = p; q < le; ++q)
        if (f[q] == '\t') { if (nf < 16) fe[nf++] = q; ++ntab; }
    if (nf < 16) fe[nf++] = le;
    // index_range: no tab -> skipped; fewer than three -> M6A_IO_EFORMAT at the line's offset
    if (ntab >= 1) {
        r.flags |= L_TAB;
        if (ntab < 3) atomicMin(bad_at, (unsigned long long)(NAMES ? 2 * p : p));
        else if (!NAMES) r.read = dev_atoll(f, fe[2] + 1, n);
        else if (!m6a_uuid::parse(f + fe[2] + 1, f + fe[3], &nm)) atomicMin(bad_at, (unsigned long long)(2 * (fe[2] + 1) + 1));
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
    if (NAMES) lname[i] = nm;
}

__global__ void flag_kernel(const LineEv *__restrict__ ev, int64_t nlines, int64_t first, int64_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i < nlines) out[i] = i >= first && (ev[i].flags & L_TAB) ? 1 : 0;
}

__global__ void compact_kernel(const int64_t *__restrict__ flag_scan, int64_t nlines, int64_t first, const LineEv *__restrict__ ev,
                               int64_t *__restrict__ vline)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= first && i < nlines && (ev[i].flags & L_TAB)) vline[flag_scan[i]] = i;
}

__device__ inline bool same_bytes(const uint8_t *f, int64_t a, int64_t b, int64_t len)
{
    for (int64_t k = 0; k < len; k++)
        if (f[a + k] != f[b + k]) return false;
    return true;
}

// valid line j starts a run when its contig bytes or its read index (NAMES: its 128-bit read name) differ from valid line j - 1's
template <bool NAMES>
__global__ void newrun_kernel(const uint8_t *__restrict__ f, const int64_t *__restrict__ nl, const LineEv *__restrict__ ev,
                              const int64_t *__restrict__ vline, int64_t NV, int64_t *__restrict__ out, const Name *__restrict__ lname)
{
    const int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (j >= NV) return;
    if (j == 0) { out[0] = 1; return; }
    const int64_t a = vline[j - 1], b = vline[j];
    const LineEv &x = ev[a], &y = ev[b];
    const bool other = NAMES ? lname[a].hi != lname[b].hi || lname[a].lo != lname[b].lo : x.read != y.read;
    out[j] = other || x.contig_len != y.contig_len || !same_bytes(f, line_start(nl, a), line_start(nl, b), y.contig_len) ? 1 : 0;
}

struct RunDev {                            // one run: lines [l0, l1], bytes [start, end)
    int64_t l0, l1, start, end, read, contig, npos;
    int32_t contig_len, status, same_contig;
};

// NAMES: a run's name is its first line's
template <bool NAMES>
__global__ void runs_kernel(const uint8_t *__restrict__ f, int64_t n, const int64_t *__restrict__ nl, int64_t NL, const LineEv *__restrict__ ev,
                            const int64_t *__restrict__ vline, int64_t NV, const int64_t *__restrict__ nr_scan, RunDev *__restrict__ runs,
                            const Name *__restrict__ lname, Name *__restrict__ rname)
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
        if (NAMES) rname[r] = lname[li];
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

// a window's kept runs to the job's run list: start / end / contig become file offsets (the window's text starts at file byte b);
// l0, l1 and the k-mer offsets of the line and position records stay the window's own, and nothing reads them after the window
__global__ void keep_runs_kernel(const RunDev *__restrict__ runs, int64_t NR, int64_t b, const int64_t *__restrict__ row_off,
                                 RunDev *__restrict__ kept, int64_t *__restrict__ row_cnt)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r >= NR) return;
    RunDev R = runs[r];
    R.start += b; R.end += b; R.contig += b;
    kept[r] = R;
    row_cnt[r] = row_off[r + 1] - row_off[r];
}

// ---- grouped input (m6a_prep_group, include/m6a.h): what is kept of the windows is cut between two of them ------------------------
// The closed prefix: one lane per segment of the kept runs (seg_first: its first run; seg_rank: its contig's number in order of first
// appearance, which the host interned from the segment's name).  The last contig stretch is the tail of segments that carry the last
// segment's rank, so the kept runs in front of it end at the first run of the highest segment g whose predecessor has another rank --
// a maximum over the segment heads, 0 where the kept runs are one stretch.
__global__ void closed_prefix_kernel(const int64_t *__restrict__ seg_first, const uint32_t *__restrict__ seg_rank, int64_t NSEG,
                                     unsigned long long *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    unsigned long long v = 0;
    if (g >= 1 && g < NSEG && seg_rank[g - 1] != seg_rank[NSEG - 1]) v = (unsigned long long)seg_first[g];
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long a = __shfl_xor(v, o);
        v = a > v ? a : v;
    }
    if ((threadIdx.x & 63) == 0 && v) atomicMax(out, v);
}

// the candidate rows of the kept runs [0, n): the sum of their row counts
__global__ void rows_before_kernel(const int64_t *__restrict__ cnt, int64_t n, unsigned long long *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    unsigned long long v = r < n ? (unsigned long long)cnt[r] : 0;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}

// The removal of the closed runs and rows: what stays of a kept array, its bytes from the first open run or row on, moves to the start
// of a new array (8 bytes a lane where the source allows it, the ragged end and the 7-byte k-mers byte by byte) and the old one is
// released.  The kept arrays hold file offsets and row counts, not offsets into each other, so nothing in them is rebased: the run
// numbers of the segments the host keeps are, there.
__global__ void keep_tail_kernel(const uint8_t *__restrict__ src, int64_t n, uint8_t *__restrict__ dst)
{
    const int64_t at = ((int64_t)blockIdx.x * kBlk + threadIdx.x) * 8;
    if (at >= n) return;
    if (((uintptr_t)src & 7) == 0 && at + 8 <= n) *(uint64_t *)(dst + at) = *(const uint64_t *)(src + at);
    else
        for (int k = 0; k < 8 && at + k < n; k++) dst[at + k] = src[at + k];
}

// The carried sites in front of a batch's: element j of the new array is element from + j of a's na elements followed by b's
template <class T>
__global__ void splice_kernel(const T *__restrict__ a, int64_t na, const T *__restrict__ b, int64_t from, int64_t n, T *__restrict__ dst)
{
    const int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (j >= n) return;
    const int64_t i = from + j;
    dst[j] = i < na ? a[i] : b[i - na];
}

// ---- a stream's windows: what the back half will ask for is saved while the window's text is there -------------------------------
// A file's back half preads the contig bytes of every segment head and hands the byte ranges of declined runs to the host half; a
// stream cannot be read again.  Per kept run: the bytes of its contig name if it can head a segment (not same_contig: the first
// run of every window is one, as run_flags_kernel sees it later), and all its bytes if it is not M6A_PREP_RUN_OK -- 0 otherwise.
// Scanned, the counts are the offsets of the window's part of the two blobs.
__global__ void save_flag_kernel(const RunDev *__restrict__ runs, int64_t NR, int64_t *__restrict__ head, int64_t *__restrict__ decl)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r >= NR) return;
    head[r] = runs[r].same_contig ? 0 : runs[r].contig_len;
    decl[r] = runs[r].status != M6A_PREP_RUN_OK ? runs[r].end - runs[r].start : 0;
}

// one workgroup per kept run, lane after lane along the bytes; a run with nothing to save (most of them) leaves at once
__global__ void save_gather_kernel(const uint8_t *__restrict__ f, const RunDev *__restrict__ runs, const int64_t *__restrict__ off, int whole,
                                   uint8_t *__restrict__ out)
{
    const int64_t r = blockIdx.x, at = off[r], len = off[r + 1] - at;
    if (len <= 0) return;
    const uint8_t *src = f + (whole ? runs[r].start : runs[r].contig);
    for (int64_t i = threadIdx.x; i < len; i += blockDim.x) out[at + i] = src[i];
}

__global__ void run_cols_kernel(const RunDev *__restrict__ runs, int64_t NR, int64_t *__restrict__ npos)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r < NR) npos[r] = runs[r].status == M6A_PREP_RUN_OK ? runs[r].npos : 0;
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

// runs of the valid lines from line `first` on (index_range): runs[NR + 1], in `m`; the three work arrays are noted in `scratch`
// lname (--read_names): the lines' names; the runs' names are then allocated like the runs and returned in rname
int find_runs(DevMem &m, hipStream_t s, const uint8_t *df, int64_t n, const int64_t *nl, int64_t NL, int64_t nlines, int64_t first,
              const LineEv *ev, RunDev *&runs, int64_t &NR, std::vector<const void *> *scratch, const Name *lname = nullptr,
              Name **rname = nullptr)
{
    int rc;
    int64_t *vflag, NV = 0;
    if ((rc = m.alloc(vflag, (size_t)nlines + 1, "valid lines"))) return rc;
    if ((rc = launch(flag_kernel, nlines, s, ev, nlines, first, vflag))) return rc;
    if ((rc = scan_total(m, vflag, nlines, s, NV))) return rc;
    int64_t *vline, *nr;
    if ((rc = m.alloc(vline, (size_t)NV + 1, "valid lines"))) return rc;
    if ((rc = m.alloc(nr, (size_t)NV + 1, "run starts"))) return rc;
    if (scratch) scratch->insert(scratch->end(), {vflag, vline, nr});
    if ((rc = launch(compact_kernel, nlines, s, vflag, nlines, first, ev, vline))) return rc;
    if ((rc = lname ? launch(newrun_kernel<true>, NV, s, df, nl, ev, vline, NV, nr, lname)
                    : launch(newrun_kernel<false>, NV, s, df, nl, ev, vline, NV, nr, nullptr)))
        return rc;
    if ((rc = scan_total(m, nr, NV, s, NR))) return rc;     // nr[j] = run of valid line j (exclusive scan of the starts) ...
    // ... so valid line j's run is nr[j + 1] - 1: shift by one with an inclusive view
    if ((rc = m.alloc(runs, (size_t)NR + 1, "runs"))) return rc;
    if (lname && (rc = m.alloc(*rname, (size_t)NR + 1, "read names"))) return rc;
    return lname ? launch(runs_kernel<true>, NV, s, df, n, nl, NL, ev, vline, NV, nr + 1, runs, lname, *rname)
                 : launch(runs_kernel<false>, NV, s, df, n, nl, NL, ev, vline, NV, nr + 1, runs, nullptr, nullptr);
}

// combine of runs[0, NR) (count, then write ps at pos_off) and the count of their candidate rows: row_off is the exclusive scan
int count_rows(DevMem &m, hipStream_t s, const uint8_t *df, const LineEv *ev, RunDev *runs, int64_t NR, int w, int64_t *&pos_off, PosRec *&ps,
               int64_t *&row_off, int64_t &NROW)
{
    int rc;
    int64_t NP = 0;
    if ((rc = m.alloc(pos_off, (size_t)NR + 1, "positions"))) return rc;
    if ((rc = launch(combine_kernel, NR, s, df, ev, runs, NR, nullptr, nullptr)) || (rc = launch(run_cols_kernel, NR, s, runs, NR, pos_off))) return rc;
    if ((rc = scan_total(m, pos_off, NR, s, NP))) return rc;
    if ((rc = m.alloc(ps, (size_t)NP + 1, "combined positions"))) return rc;
    if ((rc = m.alloc(row_off, (size_t)NR + 1, "rows"))) return rc;
    if ((rc = launch(combine_kernel, NR, s, df, ev, runs, NR, pos_off, ps)) ||
        (rc = launch(window_kernel, NR, s, df, runs, NR, pos_off, ps, w, row_off, nullptr, nullptr, nullptr, nullptr)))
        return rc;
    return scan_total(m, row_off, NR, s, NROW);
}

// The device results of the front half (upload, newline scan, lines, runs, combine, windows); all of them live in `m`.
struct Front {
    int64_t n = 0, NR = 0, NROW = 0;
    int64_t n_windows = 1, window_bytes = 0; // whole file: one window, of no set size
    RunDev *runs = nullptr;
    int64_t *row_off = nullptr, *row_pos = nullptr;
    uint8_t *row_kmer = nullptr;
    double *row_feat = nullptr;
    std::vector<const void *> scratch;      // the file, its newlines, lines and combined positions: nothing after the windows reads them
    bool bgzf_ok = false;                   // in: the caller takes BGZF input (sites_impl)
    bool read_names = false;                // in: field 4 is a read name (m6a_prep_sites_build_names)
    Name *rnames = nullptr;                 // out, read_names: [NR] the runs' names; RunDev.read is 0 until they are interned
    const uint8_t *text = nullptr;          // out, BGZF input: the inflated text, NOT in scratch -- the caller reads names and runs from it
    int64_t n_blocks = 0, comp_bytes = 0;   // out, BGZF input
    double ms_inflate = 0;
    // out, a stream (StreamSource): n is the bytes it delivered, and what the back half would read from a file again was saved from
    // every window while its text was there -- NOT in scratch, the caller releases them
    bool stream = false;
    const uint8_t *heads = nullptr;         // the contig bytes of every run that can head a segment, end to end in run order
    const uint8_t *declined = nullptr;      // the bytes [start, end) of every run that is not M6A_PREP_RUN_OK, likewise
    int64_t n_heads = 0, n_declined = 0;
};

// m6a_bgzf.h, included at the end of this file
bool bgzf_is_gzip(int fd, int64_t n);
int bgzf_front(int device_id, const char *path, int fd, int64_t n_file, DevMem &m, Streams &S, int64_t chunk, uint8_t *&text, int64_t &n_text, Front &F, double *ms);
int bgzf_gather(DevMem &m, hipStream_t s, const uint8_t *text, int64_t n_text, const std::vector<int64_t> &src, const std::vector<int64_t> &len,
                std::vector<uint8_t> &out);

// `-` is descriptor 0; whatever else fstat shows is no regular file (a FIFO, /dev/fd/N, a character device) is a stream as well
bool is_stdin(const char *path) { return path[0] == '-' && path[1] == 0; }
bool is_stream(const char *path)
{
    struct stat st;
    if (is_stdin(path) ? fstat(0, &st) != 0 : stat(path, &st) != 0) return false;      // not there: the caller's open says so
    return !S_ISREG(st.st_mode);
}

// the format error line_kernel found lowest in the text that starts at file byte b
int bad_line(const char *path, bool names, int64_t b, unsigned long long bad_at)
{
    if (names && (bad_at & 1)) return prep_fail(M6A_EFORMAT, "%s: read name at byte %lld: not a lowercase UUID", path, (long long)(b + (int64_t)(bad_at >> 1)));
    return prep_fail(M6A_EFORMAT, "%s: short line at byte %lld", path, (long long)(b + (int64_t)(names ? bad_at >> 1 : bad_at)));
}

// M6A_PREP_WINDOW_KB as a window size in bytes (unset, 0 or not a number: the whole file)
int64_t window_from_env()
{
    const char *e = getenv("M6A_PREP_WINDOW_KB");
    return e && atoll(e) > 0 ? atoll(e) << 10 : 0;
}

// One window: file bytes [b, b + n); `len` bytes from b are in df, zeros behind them.  A resident file is the one window that starts
// at 0 and is the last.
struct Win {
    const uint8_t *df = nullptr;
    int64_t b = 0, len = 0, n = 0, first = 0;
    bool last = false, grow = false;
    bool index = false;                     // in: --skip_index -- no header line is asked for, and a short line is not reported here
    int64_t NL = 0, nlines = 0, NR = 0, keep = 0, next = 0;
    int64_t *bcnt = nullptr;                // in: the newlines of every scan block, [blocks + 1]; lines_of scans them
    int64_t *nl = nullptr;
    LineEv *ev = nullptr;
    unsigned long long *bad = nullptr;      // [1] line_kernel's bad_at
    Name *lname = nullptr;                  // [nlines] with read_names
    RunDev *runs = nullptr;
    bool read_names = false;                // in: --read_names
    Name *rnames = nullptr;                 // [NR] then
};

// The line pass: from the newline counts of V's scan blocks to the newline offsets, n and the line count, the line records (and
// names) and the file's first bad line -- or V.grow, where a window that is not the last holds no newline.  t0: when the newline
// phase began (a window counts its newlines inside it).  ms[1] takes the newline part, ms[2] the lines.
int lines_of(DevMem &m, hipStream_t s, const char *path, Win &V, double t0, double *ms)
{
    int rc;
    const int64_t nb = padded(V.len) / kScanBytes;
    if ((rc = scan_total(m, V.bcnt, nb, s, V.NL))) return rc;
    if (!V.index && V.last && V.b == 0 && V.NL == 0) return prep_fail(M6A_EFORMAT, "%s: no header line", path);
    V.grow = !V.last && V.NL == 0;                           // a line longer than the window
    if (V.grow) return M6A_OK;
    if ((rc = m.alloc(V.nl, (size_t)V.NL + 1, "newline offsets"))) return rc;
    nl_write_kernel<<<(unsigned)nb, kBlk, 0, s>>>((const uint4 *)V.df, nb, V.bcnt, V.nl);
    PCHK(hipGetLastError());
    if (V.last) {                                            // the only window that may end without a newline
        uint8_t end = '\n';
        if (V.len > 0) { if ((rc = fetch(end, V.df + V.len - 1, s))) return rc; }
        else PCHK(hipStreamSynchronize(s));
        V.n = V.len;
        V.nlines = V.NL + (end != '\n' ? 1 : 0);
    } else {                                                 // it ends behind its last newline; what follows is the next window's
        int64_t at = 0;
        if ((rc = fetch(at, V.nl + V.NL - 1, s))) return rc;
        V.n = at + 1;
        V.nlines = V.NL;
    }
    ms[1] += now_ms() - t0;

    const double t1 = now_ms();
    if ((rc = m.alloc(V.ev, (size_t)std::max<int64_t>(V.nlines, 1), "line records"))) return rc;
    if ((rc = m.alloc(V.bad, 1, "flags"))) return rc;
    const unsigned long long none = ~0ull;
    PCHK(hipMemcpyAsync(V.bad, &none, sizeof none, hipMemcpyHostToDevice, s));
    if (V.read_names && (rc = m.alloc(V.lname, (size_t)std::max<int64_t>(V.nlines, 1), "read names"))) return rc;
    rc = V.lname ? launch(line_kernel<true>, V.nlines - V.first, s, V.df, V.n, V.nl, V.NL, V.nlines, V.first, V.ev, V.bad, V.lname)
                 : launch(line_kernel<false>, V.nlines - V.first, s, V.df, V.n, V.nl, V.NL, V.nlines, V.first, V.ev, V.bad, nullptr);
    if (rc) return rc;
    unsigned long long bad_at = none;
    if ((rc = fetch(bad_at, V.bad, s))) return rc;
    // every line in front of this window has been seen, so this is the file's first bad line, as whole-file mode reports it
    if (!V.index && bad_at != none) return bad_line(path, V.lname != nullptr, V.b, bad_at);
    ms[2] += now_ms() - t1;
    return M6A_OK;
}

// ---- the front half in windows ---------------------------------------------------------------------------------------------------
// The text goes through HBM W bytes at a time and only runs and candidate rows stay (include/m6a.h states the cut; the stream's
// windows are the file's, tests/window_statement.py).  Window k is bytes [b, e): e is the byte after the last '\n' among the W bytes
// from b, or the text's end in the last window; lines, runs, combine and windows are the whole-file kernels on that text (line 0 is
// the header in window 0 only).  The last run of a window that is not the last may go on behind e: it is left out, and the next window
// starts at its first byte -- so every kept run was seen whole, and a window whose only run starts at b is done again at twice the
// size.  The first run of a window has same_contig = 0: a contig cut by a window becomes two segments, which both consumers intern
// under one name, and sites_impl's rank0 of the second is the number of runs the transcript had before it (tx_runs) --
// run_select_kernel's rank0 + (r - first) is then the rank the run has in the one segment of whole-file mode, because the two segments
// are consecutive runs.
// One loop (front_windows) asks a Source for the bytes; there are two.  Two text buffers and one arena serve both: while the kernel
// stream combines and windows window k, a thread brings window k + 1 through the pinned pair and the copy stream, and the kernels of
// two windows never overlap.
//   a file     (FileSource) the thread preads.  It starts when window k's cut is known and reads from b of k + 1, so the bytes between
//              that and window k's end are read again (not copied from window k's buffer: the next text then starts 16-byte aligned
//              at its buffer's start, which the newline scan needs).  A window that grows is read again from b at twice the size.
//   a stream   (StreamSource) `--eventalign -`, a FIFO, /dev/fd/N: the text comes once and in order, and its length is known when it
//              ends.  Window k is the `size` bytes from b, the last one exactly when no byte follows them -- the reader's one byte of
//              lookahead (m6a_stream.h) answers that without consuming.  Nothing crosses the link twice:
//     carry    the bytes of window k from b of window k + 1 on (the dropped run, what lies behind the last newline) are copied device
//              to device to the start of the next buffer, which keeps the text 16-byte aligned at its base; the stream's next bytes
//              are appended behind them, so only the append position is unaligned, and zeros follow the text to a whole scan block.
//              A window that grew may leave more than W bytes: the next windows are cut from them first.
//     growth   the buffer is grown by copy and `size` more bytes are appended.
//     reading  a thread of the reader's own (m6a_stream::Ring) fills the two pinned chunks from the pipe all the time: it does not
//              wait for a cut, because the stream's order is fixed.  From the cut of window k on, the second thread takes the next
//              window's bytes out of the chunks and copies them behind the carried bytes.
//     saving   the back half cannot pread a stream: Kept::append saves the contig bytes of segment heads and the bytes of declined
//              runs from the window's text (save_flag_kernel, scan, save_gather_kernel), and sites_impl gathers from the two blobs.
// What stays is appended in place: kept runs, their row counts and the three row arrays grow as device vectors.  A file projects their
// capacity from the rows per byte so far, so the usual peak is the rows plus a margin; a stream's length is unknown, so they grow
// geometrically (twice what is needed, then DevVec::fit's fallbacks).  (Result blocks per window, flattened at the end with each block
// released as it is copied, would hold the rows twice at the moment the flat arrays are allocated.)  A vector that outgrows its
// capacity is copied into a new one and both exist during the copy: a wrong projection costs up to twice that array for that moment,
// and where the budget cannot take the projection the vector grows by half, not window by window.

// a device array that grows at its end; everything in it is counted in `m`
struct DevVec {
    uint8_t *p = nullptr;
    size_t cap = 0, used = 0;                               // bytes
    // room for `need` bytes: `hope` (the projection) if the budget allows it, else half as much again as there is, else just `need`.
    // What is there stays (s is idle); while it is copied the old and the new array both count against the budget.
    int fit(DevMem &m, size_t need, size_t hope, hipStream_t s, const char *what)
    {
        if (p && need <= cap) return M6A_OK;
        Arena *const a = m.arena;
        m.arena = nullptr;
        uint8_t *q = nullptr;
        int rc = M6A_OK;
        const size_t tries[3] = {hope, cap + cap / 2, need};
        for (size_t t : tries) {
            if (t < need || (t > need && m.used + t > m.budget)) continue;
            hope = t;
            rc = m.alloc(q, t, what);
            break;
        }
        m.arena = a;
        if (rc) return rc;
        if (used) {
            PCHK(hipMemcpyAsync(q, p, used, hipMemcpyDeviceToDevice, s));
            PCHK(hipStreamSynchronize(s));
        }
        if (p) m.release(p);
        p = q;
        cap = std::max<size_t>(16, hope);
        return M6A_OK;
    }
};

// newline count, lines and runs of a window, and its cut: n, keep (the runs that stay) and next (b of the window after) -- or grow
int window_cut(DevMem &m, hipStream_t s, const char *path, Win &V, double *ms)
{
    double t1 = now_ms();
    int rc;
    const int64_t nb = padded(V.len) / kScanBytes;
    if ((rc = m.alloc(V.bcnt, (size_t)nb + 1, "newline counts"))) return rc;
    nl_count_kernel<<<(unsigned)nb, kBlk, 0, s>>>((const uint4 *)V.df, 0, V.bcnt);
    PCHK(hipGetLastError());
    if ((rc = lines_of(m, s, path, V, t1, ms)) || V.grow) return rc;

    t1 = now_ms();
    if ((rc = find_runs(m, s, V.df, V.n, V.nl, V.NL, V.nlines, V.first, V.ev, V.runs, V.NR, nullptr, V.lname, &V.rnames))) return rc;
    V.keep = V.NR;
    V.next = V.b + V.n;
    if (!V.last && V.NR > 0) {                               // the last run may go on in the next window: that one starts with it
        int64_t start = 0;
        if ((rc = fetch(start, &V.runs[V.NR - 1].start, s))) return rc;
        V.keep = V.NR - 1;
        V.next = V.b + start;
        V.grow = V.next == V.b;                              // its only run, from its first byte: no cut in here
    }
    ms[2] += now_ms() - t1;
    return M6A_OK;
}

// a stream's window: where its kept runs' saved bytes go in the window's part of the two blobs (save_flag_kernel, scanned)
struct Save {
    int64_t *head = nullptr, *decl = nullptr;             // [keep + 1] each
    int64_t n_head = 0, n_decl = 0;
};

int save_plan(DevMem &m, hipStream_t s, const Win &V, Save &sv)
{
    int rc;
    if ((rc = m.alloc(sv.head, (size_t)V.keep + 1, "saved names")) || (rc = m.alloc(sv.decl, (size_t)V.keep + 1, "saved runs"))) return rc;
    if ((rc = launch(save_flag_kernel, V.keep, s, V.runs, V.keep, sv.head, sv.decl))) return rc;
    if ((rc = scan_total(m, sv.head, V.keep, s, sv.n_head))) return rc;
    return scan_total(m, sv.decl, V.keep, s, sv.n_decl);
}

// what stays of the windows: the job's runs, their row counts and the three row arrays, each grown at its end
struct Kept {
    DevVec runs, cnt, pos, kmer, feat, names;             // names: 16 B per kept run, --read_names only
    DevVec heads, declined;                               // a stream only: Front::heads, Front::declined
    int64_t NR = 0, NROW = 0;
    // window V's kept runs and their `nrow` rows behind what is there; `ahead` = what the whole file is expected to hold over what is held now
    // sv (a stream): the window's saved bytes go behind the two blobs, which grow as the arrays do
    int append(DevMem &m, hipStream_t s, const Win &V, int w, double ahead, const int64_t *pos_off, const PosRec *ps, const int64_t *row_off,
               int64_t nrow, const Save *sv = nullptr)
    {
        const int64_t K = 5 + 2 * w, NF = 3 * (2 * w + 1);
        const size_t nr = (size_t)(NR + V.keep) + 1, nw = (size_t)(NROW + nrow) + 1;
        int rc;
        if ((rc = runs.fit(m, nr * sizeof(RunDev), (size_t)((double)nr * ahead) * sizeof(RunDev), s, "runs")) ||
            (rc = cnt.fit(m, nr * 8, (size_t)((double)nr * ahead) * 8, s, "rows")) ||
            (rc = pos.fit(m, nw * 8, (size_t)((double)nw * ahead) * 8, s, "rows")) ||
            (rc = kmer.fit(m, nw * (size_t)K, (size_t)((double)nw * ahead) * (size_t)K, s, "rows")) ||
            (rc = feat.fit(m, nw * (size_t)NF * 8, (size_t)((double)nw * ahead) * (size_t)NF * 8, s, "rows")))
            return rc;
        if (V.rnames && (rc = names.fit(m, nr * sizeof(Name), (size_t)((double)nr * ahead) * sizeof(Name), s, "read names"))) return rc;
        if (V.rnames && V.keep)               // the dropped last run takes its name with it
            PCHK(hipMemcpyAsync((Name *)names.p + NR, V.rnames, (size_t)V.keep * sizeof(Name), hipMemcpyDeviceToDevice, s));
        if (nrow && (rc = launch(window_kernel, V.keep, s, V.df, V.runs, V.keep, pos_off, ps, w, nullptr, row_off, (int64_t *)pos.p + NROW,
                                 kmer.p + NROW * K, (double *)feat.p + NROW * NF)))
            return rc;
        if ((rc = launch(keep_runs_kernel, V.keep, s, V.runs, V.keep, V.b, row_off, (RunDev *)runs.p + NR, (int64_t *)cnt.p + NR))) return rc;
        if (sv) {
            const size_t nh = heads.used + (size_t)sv->n_head, nd = declined.used + (size_t)sv->n_decl;
            if ((rc = heads.fit(m, nh, (size_t)((double)nh * ahead), s, "saved names")) ||
                (rc = declined.fit(m, nd, (size_t)((double)nd * ahead), s, "saved runs")))
                return rc;
            if (sv->n_head) {
                save_gather_kernel<<<(unsigned)V.keep, kBlk, 0, s>>>(V.df, V.runs, sv->head, 0, heads.p + heads.used);
                PCHK(hipGetLastError());
            }
            if (sv->n_decl) {
                save_gather_kernel<<<(unsigned)V.keep, kBlk, 0, s>>>(V.df, V.runs, sv->decl, 1, declined.p + declined.used);
                PCHK(hipGetLastError());
            }
            heads.used = nh; declined.used = nd;
        }
        PCHK(hipStreamSynchronize(s));
        NR += V.keep; NROW += nrow;
        runs.used = (size_t)NR * sizeof(RunDev); cnt.used = (size_t)NR * 8;
        if (V.rnames) names.used = (size_t)NR * sizeof(Name);
        pos.used = (size_t)NROW * 8; kmer.used = (size_t)(NROW * K); feat.used = (size_t)(NROW * NF) * 8;
        return M6A_OK;
    }
};

// the thread that brings window k + 1 while window k is combined; joined where it goes out of scope
struct Upload {
    int rc = M6A_OK;
    std::string err;
    double ms = 0;
    int64_t got = 0;                        // the bytes it brought, and (a stream) whether no byte follows them
    bool eof = false;
    m6a_stream::Ring *ring = nullptr;       // a stream: left running on an error, nothing more is wanted of it
    std::thread t;
    template <class Work> void start(Work work)
    {
        t = std::thread([this, work]() {
            const double t0 = now_ms();
            rc = work();
            if (rc) err = g_prep_err;                       // the text is this thread's; the caller takes it over
            ms = now_ms() - t0;
        });
    }
    void wait() { if (t.joinable()) t.join(); }
    ~Upload() { if (t.joinable()) { if (ring) ring->abandon(); t.join(); } }
};

struct Text { uint8_t *p = nullptr; int64_t cap = 0; };

// what the window loop and its source share: the two text buffers, the arena, and what the link did
struct Windows {
    int device_id;
    const char *path;
    int64_t W, chunk;
    DevMem &m;
    Streams &S;
    const char *text_what = "";             // the source's name for a text buffer in the budget error
    Text text[2];
    Arena arena;
    double wait_ms = 0, copy_ms = 0, copied = 0;
    Windows(int device, const char *p, int64_t w, int64_t c, DevMem &mem, Streams &st) : device_id(device), path(p), W(w), chunk(c), m(mem), S(st) {}
    int text_fit(Text &T, int64_t len)      // what was in it is gone
    {
        const int64_t cap = padded(len);
        if (cap <= T.cap) return M6A_OK;
        if (T.p) m.release(T.p);
        T.p = nullptr; T.cap = 0;
        const int e = m.alloc(T.p, (size_t)cap, text_what);
        if (!e) T.cap = cap;
        return e;
    }
    int arena_grow()
    {
        PCHK(hipStreamSynchronize(S.s[0]));
        if (arena.base) m.release(arena.base);
        arena.base = nullptr;
        const size_t cap = std::max(arena.cap * 2, (arena.need + 4095) & ~(size_t)4095);
        arena.cap = arena.off = 0;
        const int e = m.alloc(arena.base, cap, "the scratch of a window");
        if (!e) arena.cap = cap;
        return e;
    }
    // the first arena, for a text of `bytes`: newline offsets and line records are about 1.5 bytes per byte of text
    int arena_start(int64_t bytes) { arena.need = (size_t)std::min(W, std::max(bytes, kScanBytes)) * 2; return arena_grow(); }
    // `bytes` arrived while the loop waited, from t0 on
    void arrived(double t0, int64_t bytes) { const double dt = now_ms() - t0; wait_ms += dt; copy_ms += dt; copied += (double)bytes; }
};

// where the windows' bytes come from: a file or a stream
struct Source {
    Windows &C;
    explicit Source(Windows &c) : C(c) {}
    virtual ~Source() {}
    virtual int first(Text &T) = 0;                                         // window 0 arrives, and the first arena is made
    virtual void extent(Win &V, int64_t Wk) const = 0;                      // V.len and V.last of the window of Wk bytes at V.b
    virtual int start_next(const Win &V, Text &T, Text &T2, Upload &up) = 0;    // V's cut is known: window k + 1 sets out for T2
    virtual int grow(const Win &V, Text &T, int64_t Wk) = 0;               // V holds no cut: Wk bytes from V.b, waited for
    virtual void advance(const Upload &) {}                                 // window k + 1 has arrived and becomes the window at hand
    virtual double ahead(const Win &V) const = 0;                           // Kept::append's projection
    virtual bool saves() const = 0;                                         // heads and declined runs are saved from the text
    virtual int finish(int64_t b, Front &F) = 0;                            // after the last window, which began at b
};

struct FileSource : Source {
    const int fd;
    const int64_t n;
    FileSource(Windows &c, int fd_, int64_t n_) : Source(c), fd(fd_), n(n_) { C.text_what = "a window of the file"; }
    int bring(Text &T, int64_t off, int64_t len)
    {
        int rc;
        if ((rc = C.text_fit(T, len))) return rc;
        const double t0 = now_ms();
        if ((rc = upload_range(C.device_id, fd, C.path, C.S, T.p, off, len, C.chunk))) return rc;
        C.arrived(t0, len);
        return M6A_OK;
    }
    int first(Text &T) override { const int rc = C.arena_start(n); return rc ? rc : bring(T, 0, std::min(C.W, n)); }
    void extent(Win &V, int64_t Wk) const override { V.last = V.b + Wk >= n; V.len = std::min(Wk, n - V.b); }
    int start_next(const Win &V, Text &, Text &T2, Upload &up) override
    {
        const int64_t off = V.next, len = std::min(C.W, n - V.next);
        const int rc = C.text_fit(T2, len);
        if (rc) return rc;
        Windows &c = C;
        uint8_t *const dst = T2.p;
        const int f = fd;
        up.got = len;
        up.start([&c, f, dst, off, len]() { return upload_range(c.device_id, f, c.path, c.S, dst, off, len, c.chunk); });
        return M6A_OK;
    }
    int grow(const Win &V, Text &T, int64_t Wk) override                   // read again from b
    {
        PCHK(hipStreamSynchronize(C.S.s[0]));
        return bring(T, V.b, std::min(Wk, n - V.b));
    }
    // rows per byte so far, carried over the whole file, and 5 % more
    double ahead(const Win &V) const override { return (double)n / (double)std::max<int64_t>(V.next, 1) * 1.05; }
    bool saves() const override { return false; }
    int finish(int64_t, Front &) override { return M6A_OK; }
};

// up to `want` bytes of the stream -> base + have on the copy stream, zeros behind the text to a whole scan block; returns when they
// have arrived.  got: how many came (fewer than `want` only at the stream's end); eof: whether no byte follows them.  The bytes come
// out of the pinned pair, which the ring's thread fills from the pipe whether or not anybody is here to take them.
int stream_fetch(int device_id, m6a_stream::Ring &ring, Streams &S, uint8_t *base, int64_t have, int64_t want, int64_t &got, bool &eof)
{
    PCHK(hipSetDevice(device_id));
    hipError_t bad = hipSuccess;
    auto copy = [&](const uint8_t *p, int64_t k, int slot, int64_t off) {
        bad = hipMemcpyAsync(base + have + off, p, (size_t)k, hipMemcpyHostToDevice, S.s[1]);
        if (bad == hipSuccess) bad = hipEventRecord(S.copied[slot], S.s[1]);
        return bad == hipSuccess;
    };
    auto settle = [&](int slot) { return (bad = hipEventSynchronize(S.copied[slot])) == hipSuccess; };
    got = 0;
    const int64_t r = ring.take(want, copy, settle);
    if (r == -2) return prep_fail(M6A_EHIP, "the copy of a window of the stream: %s", hipGetErrorString(bad));
    if (r < 0) return prep_fail(M6A_EIO, "%s", ring.R.failed ? ring.R.error.c_str() : "the stream was abandoned");
    got = r;
    const int64_t len = have + got;
    if (padded(len) > len) PCHK(hipMemsetAsync(base + len, 0, (size_t)(padded(len) - len), S.s[1]));
    PCHK(hipStreamSynchronize(S.s[1]));
    const int e = ring.at_eof();
    if (e < 0) return prep_fail(M6A_EIO, "%s", ring.R.failed ? ring.R.error.c_str() : "the stream was abandoned");
    eof = e == 1;
    return M6A_OK;
}

struct StreamSource : Source {
    const char *const advice_was;
    m6a_stream::Reader R;                                   // the caller's Fd closes the descriptor (or leaves 0 alone)
    m6a_stream::Ring ring;
    int64_t have = 0, carry = 0;                            // `have` bytes from b are in the text; `carry` of them are the next window's
    bool eof = false;                                       // no byte follows the `have` bytes from b
    StreamSource(Windows &c, int fd)
        : Source(c), advice_was(c.m.advice), R(fd, false, c.path), ring(R, (uint8_t *)c.S.pin[0], (uint8_t *)c.S.pin[1], c.chunk)
    {
        C.text_what = "a window of the stream";
        C.m.advice = "a stream is parsed in windows and what is kept of them stays on the device: give a smaller --window_mb, or write the "
                     "text to a file and run `dataprep` and then `inference` (the two-step path)";
    }
    ~StreamSource() override { C.m.advice = advice_was; }
    // the first two bytes say whether this is gzip; then window 0 arrives before anything can run
    int first(Text &T) override
    {
        int rc;
        uint8_t magic[2] = {0, 0};
        const double t0 = now_ms();
        const int64_t g = R.fill(magic, 2);
        if (g < 0) return prep_fail(M6A_EIO, "%s", R.error.c_str());
        if (g == 2 && magic[0] == 0x1f && magic[1] == 0x8b)
            return prep_fail(M6A_EINVAL, "%s is a gzip-compressed stream: compressed input from a stream is not implemented; inflate it on "
                             "the way, `bgzip -dc FILE | ... --eventalign -`, or give the BGZF file by its path", C.path);
        if ((rc = C.text_fit(T, C.W))) return rc;
        if (g) PCHK(hipMemcpyAsync(T.p, magic, (size_t)g, hipMemcpyHostToDevice, C.S.s[1]));
        PCHK(hipStreamSynchronize(C.S.s[1]));
        ring.start();                                        // from here on the reader is the thread's
        int64_t got = 0;
        if ((rc = stream_fetch(C.device_id, ring, C.S, T.p, g, C.W - g, got, eof))) return rc;
        have = g + got;
        C.arrived(t0, have);
        return C.arena_start(have);
    }
    void extent(Win &V, int64_t Wk) const override
    {
        V.len = std::min(Wk, have);                          // have > Wk: what a grown window left; Wk is whole scan blocks then
        V.last = have < Wk || (have == Wk && eof);           // the file rule b + size >= n: no byte follows these bytes
    }
    int start_next(const Win &V, Text &T, Text &T2, Upload &up) override    // the carry moves over and the next bytes set out
    {
        carry = have - (V.next - V.b);
        const int rc = C.text_fit(T2, std::max(C.W, carry));
        if (rc) return rc;
        if (carry) PCHK(hipMemcpyAsync(T2.p, T.p + (V.next - V.b), (size_t)carry, hipMemcpyDeviceToDevice, C.S.s[1]));
        Windows &c = C;
        m6a_stream::Ring &r = ring;
        uint8_t *const dst = T2.p;
        const int64_t at = carry, want = std::max<int64_t>(0, C.W - carry);
        up.ring = &ring;
        up.start([&c, &r, &up, dst, at, want]() { return stream_fetch(c.device_id, r, c.S, dst, at, want, up.got, up.eof); });
        return M6A_OK;
    }
    int grow(const Win &, Text &T, int64_t Wk) override                    // what is there stays, the rest is appended
    {
        PCHK(hipStreamSynchronize(C.S.s[0]));
        if (have >= Wk) return M6A_OK;                       // (a grown window is not the last: a byte follows what is there)
        const int64_t cap = padded(Wk);
        if (cap > T.cap) {                                   // the old and the new buffer both count while the text is copied
            uint8_t *q = nullptr;
            const int e = C.m.alloc(q, (size_t)cap, C.text_what);
            if (e) return e;
            if (have) PCHK(hipMemcpyAsync(q, T.p, (size_t)have, hipMemcpyDeviceToDevice, C.S.s[0]));
            PCHK(hipStreamSynchronize(C.S.s[0]));
            if (T.p) C.m.release(T.p);
            T.p = q; T.cap = cap;
        }
        const double t0 = now_ms();
        int64_t got = 0;
        const int rc = stream_fetch(C.device_id, ring, C.S, T.p, have, Wk - have, got, eof);
        if (rc) return rc;
        have += got;
        C.arrived(t0, got);
        return M6A_OK;
    }
    void advance(const Upload &up) override { have = carry + up.got; eof = up.eof; }
    double ahead(const Win &) const override { return 2.0; }               // the length is unknown: twice what is needed
    bool saves() const override { return true; }
    int finish(int64_t b, Front &F) override
    {
        if (R.consumed != b + have) return prep_fail(M6A_EHIP, "the windows of %s do not add up", C.path);
        F.n = R.consumed;
        F.stream = true;
        return M6A_OK;
    }
};

// The window loop, one window a step, so that a caller can stop between two windows (m6a_prep_group takes a batch there); front_windows
// runs it to the end.
struct WindowLoop {
    Windows &C;
    Source &src;
    const int w;
    const bool read_names;
    Kept kept;
    int64_t b = 0, k = 0, n_windows = 0, w_max = 0;
    bool done = false;                      // the last window has been kept
    double ahead_fixed = 0;                 // > 0: Kept::append's projection, where the kept arrays do not grow with the file (m6a_prep_group)
    WindowLoop(Windows &c, Source &s, int w_, bool names) : C(c), src(s), w(w_), read_names(names) {}
    // window 0 arrives before anything can run; from then on window k + 1 arrives under window k's combine and windows
    int start() { return src.first(C.text[0]); }
    int step(double *ms)
    {
        DevMem &m = C.m;
        hipStream_t s = C.S.s[0];
        int rc;
        Text &T = C.text[k & 1], &T2 = C.text[(k + 1) & 1];
        Upload up;                                           // of window k + 1
        bool started = false;
        int64_t Wk = C.W;
        Win V;
        for (;;) {                                           // until the arena holds the window and the window holds a cut
            V = Win();
            V.df = T.p; V.b = b; V.first = b == 0 ? 1 : 0;
            V.read_names = read_names;
            src.extent(V, Wk);
            C.arena.off = 0;
            m.arena = &C.arena;
            rc = window_cut(m, s, C.path, V, ms);
            int64_t *pos_off = nullptr, *row_off = nullptr, nrow = 0;
            PosRec *ps = nullptr;
            Save sv;
            if (!rc && !V.grow) {
                if (!V.last && !started) {                   // the cut is known: the next window sets out
                    m.arena = nullptr;
                    if ((rc = src.start_next(V, T, T2, up))) return rc;
                    m.arena = &C.arena;
                    started = true;
                }
                const double t1 = now_ms();
                rc = count_rows(m, s, V.df, V.ev, V.runs, V.keep, w, pos_off, ps, row_off, nrow);
                if (!rc && src.saves()) rc = save_plan(m, s, V, sv);
                ms[2] += now_ms() - t1;
            }
            m.arena = nullptr;
            if (rc == kArenaFull) {
                if ((rc = C.arena_grow())) return rc;
                continue;
            }
            if (rc) return rc;
            if (V.grow) {                                    // twice the window
                Wk *= 2;
                if ((rc = src.grow(V, T, Wk))) return rc;
                continue;
            }
            const double t1 = now_ms();
            if ((rc = kept.append(m, s, V, w, ahead_fixed > 0 ? ahead_fixed : src.ahead(V), pos_off, ps, row_off, nrow, src.saves() ? &sv : nullptr))) return rc;
            ms[2] += now_ms() - t1;
            break;
        }
        ++n_windows;
        w_max = std::max(w_max, Wk);
        if (started) {
            const double t0 = now_ms();
            up.wait();
            C.wait_ms += now_ms() - t0; C.copy_ms += up.ms; C.copied += (double)up.got;
            if (up.rc) { g_prep_err = up.err; return up.rc; }
        }
        if (V.last) { done = true; return M6A_OK; }
        b = V.next;
        src.advance(up);
        ++k;
        return M6A_OK;
    }
};

int front_windows(Windows &C, Source &src, int w, Front &F, double *ms)
{
    DevMem &m = C.m;
    hipStream_t s = C.S.s[0];
    WindowLoop L(C, src, w, F.read_names);
    Kept &kept = L.kept;
    int rc = L.start();
    while (!rc && !L.done) rc = L.step(ms);
    if (rc) return rc;
    if ((rc = src.finish(L.b, F))) return rc;
    // the scratch goes before the back half: X needs the room
    for (Text &T : C.text)
        if (T.p) m.release(T.p);
    m.release(C.arena.base);
    // row_off: one exclusive scan of the row counts of all runs
    const double t1 = now_ms();
    int64_t total = 0;
    if ((rc = scan_total(m, (int64_t *)kept.cnt.p, kept.NR, s, total))) return rc;
    if (total != kept.NROW) return prep_fail(M6A_EHIP, "the windows' rows do not add up");
    ms[2] += now_ms() - t1;
    ms[0] = C.wait_ms;
    ms[5] = C.copy_ms > 0 ? C.copied / (C.copy_ms * 1e6) : 0;
    F.NR = kept.NR; F.NROW = kept.NROW; F.n_windows = L.n_windows; F.window_bytes = L.w_max;
    F.runs = (RunDev *)kept.runs.p; F.row_off = (int64_t *)kept.cnt.p; F.rnames = (Name *)kept.names.p;
    F.row_pos = (int64_t *)kept.pos.p; F.row_kmer = kept.kmer.p; F.row_feat = (double *)kept.feat.p;
    F.heads = kept.heads.p; F.n_heads = (int64_t)kept.heads.used;
    F.declined = kept.declined.p; F.n_declined = (int64_t)kept.declined.used;
    return M6A_OK;
}

// The front half of one file.  istart / iend: the runs of an eventalign.index (--skip_index), or null.  ms[0..2], ms[5] as
// m6a_prep_times reports them.  A stream, or window > 0 (rounded up to whole 4 KB blocks) and no index: the text goes through in
// windows (front_windows); else it is resident, the one window that starts at 0 and is the last.
int front_half(int device_id, const char *path, int w, const std::vector<int64_t> *istart, const std::vector<int64_t> *iend, int64_t window,
               DevMem &m, Streams &S, Fd &fd, Front &F, double *ms)
{
    const bool index_path = istart != nullptr;
    int rc = open_device(device_id, m, nullptr);             // the first file of a job sets the budget
    if (rc) return rc;
    if (is_stdin(path)) { fd.fd = 0; fd.own = false; }
    else fd.fd = ::open(path, O_RDONLY);
    if (fd.fd < 0) return prep_fail(M6A_EIO, "cannot open %s", path);
    struct stat st;
    if (fstat(fd.fd, &st) != 0) return prep_fail(M6A_EIO, "cannot stat %s", path);
    const bool stream = !S_ISREG(st.st_mode);            // a regular file takes the path below untouched
    if (stream && (index_path || !F.bgzf_ok))
        return prep_fail(M6A_EINVAL, "%s is a stream: `dataprep --device gpu` and --skip_index read the file again for the index and "
                         "the rows, and a stream comes once; `eventalign_inference` reads one", path);
    int64_t n = stream ? 0 : (int64_t)st.st_size;
    const bool gz = !stream && bgzf_is_gzip(fd.fd, n);   // by content: 1f 8b.  Text takes the path below untouched.
    if (gz && !F.bgzf_ok)
        return prep_fail(M6A_EFORMAT, "%s is gzip-compressed: `dataprep --device gpu` writes an eventalign.index of offsets into the text, "
                         "which is not there; `eventalign_inference` reads BGZF directly", path);
    if (gz && !index_path && window > 0)
        return prep_fail(M6A_EINVAL, "%s: windows over compressed input are not implemented (--window_mb, M6A_PREP_WINDOW_KB); a BGZF file "
                         "must fit resident: run it without a window", path);
    F.n = n;
    int64_t nb = padded(n) / kScanBytes;                                        // 4 KB scan blocks; the buffer is padded to them
    if (stream && window <= 0) window = M6A_PREP_STREAM_WINDOW_BYTES;           // a stream is always parsed in windows
    const int64_t W = index_path || window <= 0 ? 0 : (window + kScanBytes - 1) / kScanBytes * kScanBytes;
    uint8_t *df = nullptr;
    int64_t *bcnt = nullptr;
    if (!W && !gz) {
        rc = m.alloc(df, (size_t)(nb * kScanBytes), "the file");
        if (!rc) rc = m.alloc(bcnt, (size_t)nb + 1, "newline counts");
        if (rc) return rc;
    }

    int64_t chunk = 0;
    if ((rc = S.open(W ? W : nb * kScanBytes, chunk))) return rc;
    hipStream_t s = S.s[0];                                  // kernels; S.s[1] copies
    if (W) {
        Windows C(device_id, path, W, chunk, m, S);
        if (stream) { StreamSource src(C, fd.fd); return front_windows(C, src, w, F, ms); }
        FileSource src(C, fd.fd, n);
        return front_windows(C, src, w, F, ms);
    }
    if (gz) {                                                // the compressed bytes go up, the text is inflated where the upload would have put it
        if ((rc = bgzf_front(device_id, path, fd.fd, n, m, S, chunk, df, n, F, ms))) return rc;
        F.n = n;
        nb = padded(n) / kScanBytes;
        const double t_nl = now_ms();
        if ((rc = m.alloc(bcnt, (size_t)nb + 1, "newline counts"))) return rc;
        nl_count_kernel<<<(unsigned)nb, kBlk, 0, s>>>((const uint4 *)df, 0, bcnt);
        PCHK(hipGetLastError());
        PCHK(hipStreamSynchronize(s));
        F.ms_inflate += now_ms() - t_nl;
    }

    // ---- upload: pread chunk k into one pinned buffer while chunk k - 1 is copied and counted
    const double t_up = now_ms();
    if (!gz) {
        rc = upload_range(device_id, fd.fd, path, S, df, 0, n, chunk, [&](int slot, int64_t off, int64_t len) -> int {
            PCHK(hipStreamWaitEvent(s, S.copied[slot], 0));
            const int64_t b0 = off / kScanBytes, b1 = std::min(nb, (off + len + kScanBytes - 1) / kScanBytes);
            nl_count_kernel<<<(unsigned)(b1 - b0), kBlk, 0, s>>>((const uint4 *)df, b0, bcnt);
            PCHK(hipGetLastError());
            return M6A_OK;
        });
        if (rc) return rc;
    }
    if (n == 0) PCHK(hipMemsetAsync(bcnt, 0, sizeof(int64_t), s));
    PCHK(hipStreamSynchronize(S.s[1]));
    PCHK(hipStreamSynchronize(s));
    if (!gz) {
        ms[0] = now_ms() - t_up;
        ms[5] = ms[0] > 0 ? (double)n / (ms[0] * 1e6) : 0;
    }

    // ---- newline offsets and lines
    Win V;
    V.df = df; V.len = n; V.last = true; V.first = 1; V.index = index_path; V.bcnt = bcnt;
    V.read_names = F.read_names;
    if ((rc = lines_of(m, s, path, V, now_ms(), ms))) return rc;

    // ---- runs, combine, windows
    const double t1 = now_ms();
    int64_t NR = 0;
    RunDev *runs = nullptr;
    if (!index_path) {
        if ((rc = find_runs(m, s, df, n, V.nl, V.NL, V.nlines, 1, V.ev, runs, NR, &F.scratch, V.lname, &F.rnames))) return rc;
    } else {
        NR = (int64_t)istart->size();
        if ((rc = m.alloc(runs, (size_t)NR + 1, "runs"))) return rc;
        std::vector<RunDev> h((size_t)NR);
        for (int64_t r = 0; r < NR; r++) { h[(size_t)r].start = (*istart)[(size_t)r]; h[(size_t)r].end = (*iend)[(size_t)r]; }
        if (NR) PCHK(hipMemcpyAsync(runs, h.data(), (size_t)NR * sizeof(RunDev), hipMemcpyHostToDevice, s));
        if ((rc = launch(runs_from_index_kernel, NR, s, n, V.nl, V.NL, V.nlines, runs, NR))) return rc;
        PCHK(hipStreamSynchronize(s));                        // h goes out of scope
    }
    int64_t *pos_off, *row_off, NROW = 0;
    PosRec *ps;
    if ((rc = count_rows(m, s, df, V.ev, runs, NR, w, pos_off, ps, row_off, NROW))) return rc;
    const int64_t K = 5 + 2 * w, NF = 3 * (2 * w + 1);
    int64_t *drow_pos;
    uint8_t *drow_kmer;
    double *drow_feat;
    if ((rc = m.alloc(drow_pos, (size_t)NROW, "rows"))) return rc;
    if ((rc = m.alloc(drow_kmer, (size_t)(NROW * K), "rows"))) return rc;
    if ((rc = m.alloc(drow_feat, (size_t)(NROW * NF), "rows"))) return rc;
    if (NROW && (rc = launch(window_kernel, NR, s, df, runs, NR, pos_off, ps, w, nullptr, row_off, drow_pos, drow_kmer, drow_feat))) return rc;
    PCHK(hipStreamSynchronize(s));
    ms[2] += now_ms() - t1;
    F.NR = NR; F.NROW = NROW; F.runs = runs; F.row_off = row_off; F.row_pos = drow_pos; F.row_kmer = drow_kmer; F.row_feat = drow_feat;
    F.scratch.insert(F.scratch.end(), {bcnt, V.nl, V.ev, V.bad, pos_off, ps});
    if (V.lname) F.scratch.push_back(V.lname);
    if (gz) F.text = df;
    else F.scratch.push_back(df);
    return M6A_OK;
}

int prep_impl(int device_id, const char *path, int w, const char *index_path, m6a_prep &P)
{
    if (w < 1 || w > 16) return prep_fail(M6A_EINVAL, "n_neighbors must be 1..16");
    if (is_stream(path))                                    // before anything is opened: opening a FIFO waits for its writer
        return prep_fail(M6A_EINVAL, "%s is a stream: `dataprep --device gpu` and --skip_index read the file again for the index and the "
                         "rows, and a stream comes once; `eventalign_inference` reads one", path);
    // --skip_index: the runs come from the file (read before anything touches the device, as the host path does)
    std::vector<std::string> names;
    std::vector<uint32_t> itx;
    std::vector<int64_t> iread, istart, iend;
    if (index_path) {
        int rc = read_index(index_path, names, itx, iread, istart, iend);
        if (rc) return rc;
    }
    DevMem m;
    Streams S;
    Fd fd;
    Front F;
    // an index's rows are arbitrary byte ranges, so --skip_index keeps the file resident whatever M6A_PREP_WINDOW_KB says
    int rc = front_half(device_id, path, w, index_path ? &istart : nullptr, index_path ? &iend : nullptr, index_path ? 0 : window_from_env(),
                        m, S, fd, F, P.ms);
    if (rc) return rc;
    hipStream_t s = S.s[0];
    const int64_t NR = F.NR, NROW = F.NROW, K = 5 + 2 * w, NF = 3 * (2 * w + 1);
    RunDev *runs = F.runs;
    const int64_t *row_off = F.row_off, *drow_pos = F.row_pos;
    const uint8_t *drow_kmer = F.row_kmer;
    const double *drow_feat = F.row_feat;
    double t1;

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
        Interner tx(P.blob, P.tx_off);
        std::string nm;
        uint32_t cur = 0;
        for (int64_t r = 0; r < NR; r++) {
            const RunDev &R = hr[(size_t)r];
            if (r == 0 || !R.same_contig) {
                nm.resize((size_t)R.contig_len);
                if ((rc = read_fully(fd.fd, &nm[0], R.contig_len, R.contig, path))) return rc;
                cur = tx.id(nm);
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

// ---- the back half (m6a_prep_sites): the candidate rows, still in HBM, -> the arrays m6a_io_load_sites makes of data.json -------
// What m6a_io_dataprep_write's preprocess_transcript_rows / emit_transcript and then the loader do, on the device:
//   segments   runs where the contig bytes change; the host interns their names (transcript ids in order of first appearance)
//              and gives every segment its transcript, the rank of its first run inside the transcript and the readcount verdict
//   runs       a run is used when its rank <= readcount_max, its transcript has >= readcount_min counted runs and npos > 1; of
//              the runs of one (transcript, read) the last supplies the rows and the first the place (a Python dict's overwrite)
//   rows       the used runs' rows sorted by (transcript, position, place) -- LSD radix sort, 4-bit digits, stable
//   sites      cut where (transcript, position) changes; 7-mers must agree; kept with >= min_segment_count and >= 20 reads
//   X          (float)((v - mean) / std) in f64 per feature, as m6a_io_load_sites computes it
namespace {

// flag[i] -> list of the flagged i (after the exclusive scan of the flags: ex[i + 1] != ex[i])
__global__ void compact_u32_kernel(const int64_t *__restrict__ ex, int64_t n, uint32_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i < n && ex[i + 1] != ex[i]) out[ex[i]] = (uint32_t)i;
}

struct SegDev { int64_t first, contig; int32_t len, pad; };        // a segment: runs from `first` on with the same contig bytes
struct SegUp { int64_t rank0; uint32_t tx, keep; };                  // from the host: its transcript and the rank of its first run
struct DeclDev { int64_t run, start, end, read; };                   // a run the front half declined
struct DeclUp { int64_t run, npos; };

__global__ void run_flags_kernel(const RunDev *__restrict__ runs, int64_t NR, int64_t *__restrict__ seg, int64_t *__restrict__ decl)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r >= NR) return;
    seg[r] = r == 0 || !runs[r].same_contig;
    decl[r] = runs[r].status != M6A_PREP_RUN_OK;
}

__global__ void run_lists_kernel(const RunDev *__restrict__ runs, int64_t NR, const int64_t *__restrict__ sx, const int64_t *__restrict__ dx,
                                 SegDev *__restrict__ seg, DeclDev *__restrict__ decl)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r >= NR) return;
    const RunDev &R = runs[r];
    if (sx[r + 1] != sx[r]) seg[sx[r]] = SegDev{r, R.contig, R.contig_len, 0};
    if (dx[r + 1] != dx[r]) decl[dx[r]] = DeclDev{r, R.start, R.end, R.read};
}

__global__ void decl_patch_kernel(RunDev *__restrict__ runs, const DeclUp *__restrict__ up, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    runs[up[i].run].npos = up[i].npos;
    runs[up[i].run].status = M6A_PREP_RUN_OK;
}

// preprocess_transcript_rows' loop: counted (rank <= lim), transcript kept, `if data.size > 1`
__global__ void run_select_kernel(const RunDev *__restrict__ runs, int64_t NR, const int64_t *__restrict__ sx, const SegDev *__restrict__ seg,
                                  const SegUp *__restrict__ up, int64_t lim, uint32_t *__restrict__ run_tx, int64_t *__restrict__ run_rank,
                                  int64_t *__restrict__ elig)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r >= NR) return;
    const int64_t g = sx[r + 1] - 1;
    const int64_t rank = up[g].rank0 + (r - seg[g].first);
    run_tx[r] = up[g].tx;
    run_rank[r] = rank;
    elig[r] = up[g].keep && rank <= lim && runs[r].status == M6A_PREP_RUN_OK && runs[r].npos > 1;
}

struct RowSrc {                            // rows [0, n0) are the front half's, the rest the host half's (declined runs)
    const int64_t *pos0, *pos1;
    const uint8_t *kmer0, *kmer1;
    const double *feat0, *feat1;
    int64_t n0;
    __device__ int64_t pos(int64_t k) const { return k < n0 ? pos0[k] : pos1[k - n0]; }
    __device__ const uint8_t *kmer(int64_t k) const { return k < n0 ? kmer0 + k * 7 : kmer1 + (k - n0) * 7; }
    __device__ const double *feat(int64_t k) const { return k < n0 ? feat0 + k * 9 : feat1 + (k - n0) * 9; }
};

__device__ inline uint64_t bias(int64_t v) { return (uint64_t)v ^ (1ull << 63); }   // order-preserving int64 -> uint64

// min / max of runs[idx[i]].read (what == 0) or rs.pos(idx[i]) (what == 1), biased: mm[0] = min, mm[1] = max
__global__ void minmax_kernel(const uint32_t *__restrict__ idx, int64_t n, int what, const RunDev *__restrict__ runs, RowSrc rs,
                              unsigned long long *__restrict__ mm)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    unsigned long long lo = ~0ull, hi = 0;
    if (i < n) lo = hi = bias(what == 0 ? runs[idx[i]].read : rs.pos(idx[i]));
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) { atomicMin(&mm[0], lo); atomicMax(&mm[1], hi); }
}

// the key of run E[i]: transcript << read_bits | (read - read_min); use: 1 = the read part, 2 = the transcript part
__global__ void run_key_kernel(const uint32_t *__restrict__ E, int64_t n, const RunDev *__restrict__ runs, const uint32_t *__restrict__ run_tx,
                               uint64_t read_min, int tx_shift, unsigned use, uint64_t *__restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = E[i];
    uint64_t v = 0;
    if (use & 1) v |= bias(runs[r].read) - read_min;
    if (use & 2) v |= (uint64_t)run_tx[r] << tx_shift;
    key[i] = v;
}

// E sorted by (transcript, read, rank): the last run of a group supplies the rows, the first its place
__global__ void dup_head_kernel(const uint32_t *__restrict__ E, int64_t n, const RunDev *__restrict__ runs, const uint32_t *__restrict__ run_tx,
                                int64_t *__restrict__ head)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    head[i] = i == 0 || run_tx[E[i]] != run_tx[E[i - 1]] || runs[E[i]].read != runs[E[i - 1]].read;
}

__global__ void dup_first_kernel(const uint32_t *__restrict__ E, int64_t n, const int64_t *__restrict__ gx, const int64_t *__restrict__ run_rank,
                                 int64_t *__restrict__ gfirst)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i < n && gx[i + 1] != gx[i]) gfirst[gx[i]] = run_rank[E[i]];
}

__global__ void dup_last_kernel(const uint32_t *__restrict__ E, int64_t n, const int64_t *__restrict__ gx, const int64_t *__restrict__ gfirst,
                                uint8_t *__restrict__ used, int64_t *__restrict__ run_place)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1 || gx[i + 2] != gx[i + 1]) {
        used[E[i]] = 1;
        run_place[E[i]] = gfirst[gx[i + 1] - 1];
    }
}

__global__ void used_rows_count_kernel(const uint8_t *__restrict__ used, const int64_t *__restrict__ row_off, int64_t NR, int64_t *__restrict__ cnt)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r < NR) cnt[r] = used[r] ? row_off[r + 1] - row_off[r] : 0;
}

__global__ void used_rows_write_kernel(const uint8_t *__restrict__ used, const int64_t *__restrict__ row_off, int64_t NR, const int64_t *__restrict__ ex,
                                       uint32_t *__restrict__ L, uint32_t *__restrict__ row_run)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r >= NR || !used[r]) return;
    for (int64_t k = row_off[r], o = ex[r]; k < row_off[r + 1]; k++, o++) {
        L[o] = (uint32_t)k;
        row_run[k] = (uint32_t)r;
    }
}

// the host half's rows: appended behind the front half's
__global__ void host_flag_kernel(const uint8_t *__restrict__ used, const int64_t *__restrict__ hrun, int64_t NH, int64_t *__restrict__ flag)
{
    const int64_t h = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (h < NH) flag[h] = used[hrun[h]];
}

__global__ void host_rows_kernel(const int64_t *__restrict__ hrun, int64_t NH, int64_t n0, int64_t L0, const int64_t *__restrict__ ex,
                                 uint32_t *__restrict__ L, uint32_t *__restrict__ row_run)
{
    const int64_t h = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (h >= NH) return;
    row_run[n0 + h] = (uint32_t)hrun[h];
    if (ex[h + 1] != ex[h]) L[L0 + ex[h]] = (uint32_t)(n0 + h);
}

struct RowKey { uint64_t pos_min; int sh_tx, sh_pos, sh_place; unsigned use; };   // use: 1 transcript, 2 position, 4 place

__global__ void row_key_kernel(const uint32_t *__restrict__ L, int64_t n, RowSrc rs, const uint32_t *__restrict__ row_run,
                               const uint32_t *__restrict__ run_tx, const int64_t *__restrict__ run_place, RowKey k, uint64_t *__restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = L[i], r = row_run[row];
    uint64_t v = 0;
    if (k.use & 1) v |= (uint64_t)run_tx[r] << k.sh_tx;
    if (k.use & 2) v |= (bias(rs.pos(row)) - k.pos_min) << k.sh_pos;
    if (k.use & 4) v |= (uint64_t)run_place[r] << k.sh_place;
    key[i] = v;
}

__global__ void site_head_kernel(const uint32_t *__restrict__ L, int64_t n, RowSrc rs, const uint32_t *__restrict__ row_run,
                                 const uint32_t *__restrict__ run_tx, int64_t *__restrict__ head)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    head[i] = i == 0 || run_tx[row_run[L[i]]] != run_tx[row_run[L[i - 1]]] || rs.pos(L[i]) != rs.pos(L[i - 1]);
}

__global__ void site_start_kernel(const int64_t *__restrict__ hx, int64_t n, int64_t *__restrict__ start)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    if (hx[i + 1] != hx[i]) start[hx[i]] = i;
    if (i == n - 1) start[hx[n]] = n;
}

// emit_transcript: every read of a site carries the site's 7-mer (else M6A_IO_EFORMAT at the first such site)
__global__ void site_check_kernel(const uint32_t *__restrict__ L, int64_t n, RowSrc rs, const int64_t *__restrict__ hx,
                                  const int64_t *__restrict__ start, unsigned long long *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    const int64_t s = hx[i + 1] - 1;
    const uint8_t *a = rs.kmer(L[i]), *b = rs.kmer(L[start[s]]);
    for (int k = 0; k < 7; k++)
        if (a[k] != b[k]) { atomicMin(bad, (unsigned long long)s); return; }
}

__global__ void probe_kernel(const uint32_t *__restrict__ L, const int64_t *__restrict__ start, int64_t s, RowSrc rs,
                             const uint32_t *__restrict__ row_run, const uint32_t *__restrict__ run_tx, int64_t *__restrict__ out)
{
    const uint32_t k = L[start[s]];
    out[0] = run_tx[row_run[k]];
    out[1] = rs.pos(k);
}

__global__ void site_keep_kernel(const int64_t *__restrict__ start, int64_t NS, int64_t need, int64_t *__restrict__ flag)
{
    const int64_t s = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (s < NS) flag[s] = start[s + 1] - start[s] >= need;
}

__global__ void site_emit_kernel(const int64_t *__restrict__ start, int64_t NS, const int64_t *__restrict__ kx, int64_t *__restrict__ src,
                                 int64_t *__restrict__ cnt)
{
    const int64_t s = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (s >= NS || kx[s + 1] == kx[s]) return;
    src[kx[s]] = start[s];
    cnt[kx[s]] = start[s + 1] - start[s];
}

__device__ inline uint64_t pack5(const uint8_t *k)
{
    return ((uint64_t)k[0] << 32) | ((uint64_t)k[1] << 24) | ((uint64_t)k[2] << 16) | ((uint64_t)k[3] << 8) | (uint64_t)k[4];
}

__device__ inline int find5(const uint64_t *keys, int n, uint64_t v)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (keys[m] < v) lo = m + 1; else hi = m; }
    return lo < n && keys[lo] == v ? lo : -1;
}

// per kept site: transcript, position, 7-mer; the norm rows and the vocabulary ids of its three 5-mers (m6a_io_load_sites' order
// of checks: the normalisation factors of the three 5-mers, then the vocabulary); bad = 8 site + what.  Pooling replicates
// (tx_map: this file's transcript ids -> the job's; defer): nothing is an error yet -- a site may still be dropped by the pooled
// filter -- so a 5-mer without factors takes row 0 (pool_site_kernel refuses the site before its X is read) and no vocabulary id is made
__global__ void site_info_kernel(const uint32_t *__restrict__ L, const int64_t *__restrict__ src, int64_t S, RowSrc rs,
                                 const uint32_t *__restrict__ row_run, const uint32_t *__restrict__ run_tx, const uint64_t *__restrict__ nkeys,
                                 const int32_t *__restrict__ nix, int n_norm, const uint64_t *__restrict__ vocab, int n_vocab,
                                 int32_t *__restrict__ site_norm,
                                 uint8_t *__restrict__ site_kmers, uint32_t *__restrict__ site_tx, int64_t *__restrict__ site_pos,
                                 uint8_t *__restrict__ site_k7, unsigned long long *__restrict__ bad, const uint32_t *__restrict__ tx_map, int defer)
{
    const int64_t s = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (s >= S) return;
    const uint32_t k = L[src[s]];
    const uint8_t *km = rs.kmer(k);
    site_tx[s] = tx_map ? tx_map[run_tx[row_run[k]]] : run_tx[row_run[k]];
    site_pos[s] = rs.pos(k);
    for (int c = 0; c < 7; c++) site_k7[s * 7 + c] = km[c];
    for (int c = 0; c < 3; c++) {
        site_norm[s * 3 + c] = 0;
        if (!n_norm) continue;
        const int j = find5(nkeys, n_norm, pack5(km + c));
        if (j < 0 && defer) continue;
        if (j < 0) { atomicMin(bad, (unsigned long long)(s * 8 + c)); return; }
        site_norm[s * 3 + c] = nix[j];
    }
    if (defer) return;
    for (int c = 0; c < 3; c++) {
        const int v = find5(vocab, n_vocab, pack5(km + c));
        if (v < 0) { atomicMin(bad, (unsigned long long)(s * 8 + 3 + c)); return; }
        site_kmers[s * 3 + c] = (uint8_t)v;
    }
}

// one lane per read of the kept sites: X[i][9] and the read id
__global__ void x_kernel(const uint32_t *__restrict__ L, const int64_t *__restrict__ src, const int64_t *__restrict__ off, int64_t S, int64_t R,
                         RowSrc rs, const uint32_t *__restrict__ row_run, const RunDev *__restrict__ runs, const int32_t *__restrict__ site_norm,
                         const double *__restrict__ nmean, const double *__restrict__ nstd, int n_norm, float *__restrict__ X,
                         double *__restrict__ read_ids)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= R) return;
    int64_t lo = 0, hi = S - 1;                          // the site s with off[s] <= i < off[s + 1]
    while (lo < hi) { const int64_t m = (lo + hi + 1) >> 1; if (off[m] <= i) lo = m; else hi = m - 1; }
    const int64_t s = lo;
    const uint32_t k = L[src[s] + (i - off[s])];
    const double *f = rs.feat(k);
    for (int c = 0; c < 3; c++) {
        const int64_t nr = 3 * (int64_t)site_norm[s * 3 + c];
        for (int q = 0; q < 3; q++) {
            double v = f[3 * c + q];
            if (v != v) v = __longlong_as_double(0x7ff8000000000000ll);      // the NaN json.loads / the loader make of "NaN"
            X[i * 9 + 3 * c + q] = n_norm ? (float)((v - nmean[nr + q]) / nstd[nr + q]) : (float)v;
        }
    }
    read_ids[i] = (double)runs[row_run[k]].read;
}

const unsigned long long kMinMax0[2] = {~0ull, 0}, kNone = ~0ull;

// `dataprep --writer device` (m6a_dataprep.h, included at the end of this file): what sites_impl hands to the writer
struct DataprepJob { const char *out_dir; int compress, n_threads; m6a_dataprep_stats *st; };
struct JsonDev {                           // device pointers: the back half's sorted rows and kept sites
    const uint32_t *L;                     // [NL] candidate rows sorted by (transcript, position, place)
    const int64_t *src, *off;              // [S] where site i starts in L; [S + 1] its reads are off[i + 1] - off[i]
    RowSrc rs;
    const uint32_t *row_run;               // row -> run
    const RunDev *runs;
    const uint32_t *site_tx;               // [S]
    const int64_t *site_pos;               // [S]
    const uint8_t *site_k7;                // [S][7]
    const uint8_t *tx_blob;
    const int64_t *tx_off;
    int round3;                            // --compress
};

struct DataprepSrc {
    JsonDev json;                          // tx_blob, tx_off and round3 are the writer's to fill
    const uint32_t *run_tx;                // [NR]
    int64_t NS, NR, NL, NT;
    const std::string *blob;               // the transcript names on the host
    const std::vector<int64_t> *tx_off;    // [NT + 1]
};
int dataprep_emit(DevMem &m, hipStream_t s0, const DataprepJob &job, const DataprepSrc &src);

int bits_for(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

// ---- read names interned (m6a_prep_sites_build_names) -------------------------------------------------------------------------------
// After the last window of a file and before anything reads RunDev.read, every run's 128-bit name becomes the dense index of the
// name in order of first appearance -- the read index the twin file (names replaced by 0, 1, ...) carries in field 4:
//   sort      the run numbers by name: LSD passes of radix_sort over lo, then hi; stable, so a group's runs stay in file order
//   heads     where the name differs from the one before; a head is its group's smallest run number
//   rank      a flag on every run that is such a first run, scanned over the run numbers: the groups in order of first appearance
//   scatter   every run takes its group's rank as RunDev.read; every head writes its name to row `rank` of the table [n][16]
// The number of names stays on the device (rank[NR]) until sites_impl fetches it together with the segment count.
struct Intern {
    uint32_t *val = nullptr;                // [NR] run numbers sorted by name
    int64_t *gx = nullptr, *rank = nullptr; // [NR + 1] exclusive scans: group heads over the sorted order, first runs over the runs
};

__global__ void name_key_kernel(const Name *__restrict__ rn, int64_t n, int hi, uint32_t *__restrict__ val, uint64_t *__restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    if (!hi) val[i] = (uint32_t)i;
    key[i] = hi ? rn[val[i]].hi : rn[i].lo;
}

__global__ void name_head_kernel(const uint32_t *__restrict__ val, int64_t n, const Name *__restrict__ rn, int64_t *__restrict__ head)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    head[i] = i == 0 || rn[val[i]].hi != rn[val[i - 1]].hi || rn[val[i]].lo != rn[val[i - 1]].lo;
}

__global__ void name_first_kernel(const uint32_t *__restrict__ val, int64_t n, const int64_t *__restrict__ gx, uint32_t *__restrict__ gfirst,
                                  int64_t *__restrict__ first)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n || gx[i + 1] == gx[i]) return;
    gfirst[gx[i]] = val[i];
    first[val[i]] = 1;
}

__global__ void name_index_kernel(const uint32_t *__restrict__ val, int64_t n, const int64_t *__restrict__ gx, const uint32_t *__restrict__ gfirst,
                                  const int64_t *__restrict__ rank, RunDev *__restrict__ runs)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i < n) runs[val[i]].read = rank[gfirst[gx[i + 1] - 1]];
}

__global__ void name_table_kernel(const uint32_t *__restrict__ val, int64_t n, const int64_t *__restrict__ gx, const int64_t *__restrict__ rank,
                                  const Name *__restrict__ rn, int64_t n_names, uint8_t *__restrict__ table)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n || gx[i + 1] == gx[i]) return;
    const int64_t k = rank[val[i]];
    if (k < n_names) m6a_uuid::to_bytes(rn[val[i]].hi, rn[val[i]].lo, table + k * 16);
}

// two counts below 2^32, each the total an exclusive scan left behind its array, as one word
__global__ void pack_totals_kernel(const int64_t *__restrict__ lo, const int64_t *__restrict__ hi, uint64_t *__restrict__ out)
{
    out[0] = (uint64_t)lo[0] | (uint64_t)hi[0] << 32;
}

int intern_runs(DevMem &m, hipStream_t s, RunDev *runs, const Name *rn, int64_t NR, Intern &in)
{
    int rc;
    uint64_t *k1, *k2;
    uint32_t *val, *val2, *gfirst;
    if ((rc = m.alloc(k1, (size_t)NR + 1, "read names")) || (rc = m.alloc(k2, (size_t)NR + 1, "read names")) ||
        (rc = m.alloc(val, (size_t)NR + 1, "read names")) || (rc = m.alloc(val2, (size_t)NR + 1, "read names")))
        return rc;
    for (int hi = 0; hi < 2 && NR; hi++)
        if ((rc = launch(name_key_kernel, NR, s, rn, NR, hi, val, k1)) || (rc = radix_sort(m, k1, val, k2, val2, NR, 64, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    m.release({k1, k2, val2});
    if ((rc = m.alloc(in.gx, (size_t)NR + 1, "read names")) || (rc = m.alloc(in.rank, (size_t)NR + 1, "read names")) ||
        (rc = m.alloc(gfirst, (size_t)NR + 1, "read names")))
        return rc;
    PCHK(hipMemsetAsync(in.gx + NR, 0, sizeof(int64_t), s));
    PCHK(hipMemsetAsync(in.rank, 0, (size_t)(NR + 1) * sizeof(int64_t), s));
    if ((rc = launch(name_head_kernel, NR, s, val, NR, rn, in.gx)) || (rc = scan_excl(m, in.gx, NR + 1, s))) return rc;
    if ((rc = launch(name_first_kernel, NR, s, val, NR, in.gx, gfirst, in.rank)) || (rc = scan_excl(m, in.rank, NR + 1, s))) return rc;
    if ((rc = launch(name_index_kernel, NR, s, val, NR, in.gx, gfirst, in.rank, runs))) return rc;
    PCHK(hipStreamSynchronize(s));
    m.release(gfirst);
    in.val = val;
    return M6A_OK;
}

// scan_total of a[0..n), and with the same 8 bytes the number of names intern_runs left at in.rank[n] (both are at most n < 2^32)
int scan_total_and_names(DevMem &m, int64_t *a, int64_t n, hipStream_t s, int64_t &total, const Intern &in, int64_t &n_names)
{
    PCHK(hipMemsetAsync(a + n, 0, sizeof(int64_t), s));
    int rc = scan_excl(m, a, n + 1, s);
    if (rc) return rc;
    uint64_t *w, h = 0;
    if ((rc = m.alloc(w, 1, "flags"))) return rc;
    pack_totals_kernel<<<1, 1, 0, s>>>(a + n, in.rank + n, w);
    PCHK(hipGetLastError());
    if ((rc = fetch(h, w, s))) return rc;
    total = (int64_t)(h & 0xffffffffull);
    n_names = (int64_t)(h >> 32);
    return M6A_OK;
}

}  // namespace

struct m6a_prep_sites;

namespace {

// what stays of one replicate until the replicates are pooled: its sites with >= min_segment_count reads (transcript ids are the
// job's), and X and the read id of their reads in site order -- 44 B per read, 31 B per site
struct FilePart {
    int64_t NC = 0, RC = 0;
    float *X = nullptr;            // [RC][9]
    double *ids = nullptr;         // [RC]
    uint32_t *tx = nullptr;        // [NC]
    int64_t *pos = nullptr, *off = nullptr;   // [NC], [NC + 1]
    uint8_t *k7 = nullptr;         // [NC][7]
    uint8_t *names = nullptr;      // [n_names][16] the file's read names in index order (--read_names)
    int64_t n_names = 0;
};

struct Pool {
    Interner tx;                                            // transcript names of all files, in order of first appearance: the job's
    std::vector<FilePart> parts;
    Pool(std::string &blob, std::vector<int64_t> &tx_off) : tx(blob, tx_off) {}
};

}  // namespace

struct m6a_prep_sites {
    m6a_prep_sites_info info{};
    int device = 0;
    std::vector<void *> dev;                 // X, site_kmers, off, read_prob, site_prob, mod_ratio, and what the CSV writer reads:
    const uint32_t *csv_tx = nullptr;        // [S] transcript of each site      } as the build left them on the device
    const int64_t *csv_pos = nullptr;        // [S] position                     } (m6a_prep_sites_write_csv, m6a_csv.h)
    const uint8_t *csv_k7 = nullptr;         // [S][7] 7-mer
    const double *csv_ids = nullptr;         // [R] read ids
    const int32_t *csv_parts = nullptr;      // [S][n_rep] reads of each site by replicate (several files)
    size_t held = 0;                         // bytes of `dev`
    std::vector<int64_t> off, pos, tx_off;
    std::vector<uint32_t> tx;
    std::vector<char> k7;
    std::string blob;
    std::vector<double> ids;
    std::vector<int32_t> rep;                // [R] replicate of each read (several files)
    // --read_names: the files' tables of names, concatenated -- file f's are rows [name_off[f], name_off[f + 1]), 16 bytes each
    bool read_names = false;
    std::vector<uint8_t> names16;
    std::vector<int64_t> name_off{0};
    const uint8_t *csv_names = nullptr;      // the same on the device, for the CSV kernels
    const int64_t *csv_name_off = nullptr;   // [n_rep + 1]
    double ms_intern = 0;
    int64_t stream_bytes = 0, n_streams = 0; // bytes read from streams, and how many of the files were streams
    // a batch of m6a_prep_group: the group counts the handle's device bytes against its budget until the handle is freed
    void (*on_free)(void *owner, size_t bytes) = nullptr;
    void *owner = nullptr;
    ~m6a_prep_sites()
    {
        for (void *p : dev) (void)hipFree(p);
        if (on_free) on_free(owner, held);
    }
};

namespace {

// the error of the lowest bad site (8 site + what) that site_info_kernel or, pooled, pool_site_kernel found; the sites are in P
int bad_site(const m6a_prep_sites &P, unsigned long long bad, bool pooled)
{
    const int64_t bs = (int64_t)(bad >> 3), what = (int64_t)(bad & 7);
    const char *k = P.k7.data() + bs * 7;
    if (what < 3) return prep_fail(M6A_EFORMAT, "no normalisation factors for %.5s", k + what);
    const uint32_t t = P.tx[(size_t)bs];
    const int len = (int)(P.tx_off[t + 1] - P.tx_off[t]);
    if (pooled && what == 3)
        return prep_fail(M6A_EFORMAT, "replicates disagree on the sequence of %.*s:%lld", len, P.blob.data() + P.tx_off[t], (long long)P.pos[(size_t)bs]);
    return prep_fail(M6A_EFORMAT, "site %.*s:%lld: %.7s is not a DRACH context", len, P.blob.data() + P.tx_off[t], (long long)P.pos[(size_t)bs], k);
}

// what the build leaves on the device becomes P's: out of `m`, into P.dev, and under the names the model and the CSV writer read
struct Result {
    int64_t NS, R, NT;
    int n_rep;
    float *X;
    uint8_t *site_kmers;
    int64_t *off;
    float *read_prob, *site_prob;
    double *mod_ratio;
    const uint32_t *site_tx;
    const int64_t *site_pos;
    const uint8_t *site_k7;
    const double *ids;
    const int32_t *parts;                   // several files, else null
    const uint8_t *names;                   // --read_names, else null
    const int64_t *name_off;
};

void publish(m6a_prep_sites &P, DevMem &m, const Result &r)
{
    for (const void *p : std::initializer_list<const void *>{r.X, r.site_kmers, r.off, r.read_prob, r.site_prob, r.mod_ratio, r.site_tx, r.site_pos,
                                                             r.site_k7, r.ids, r.parts, r.names, r.name_off}) {
        if (!p) continue;
        P.held += m.size_of(p);
        m.detach(p);
        P.dev.push_back((void *)p);
    }
    P.csv_tx = r.site_tx; P.csv_pos = r.site_pos; P.csv_k7 = r.site_k7; P.csv_ids = r.ids; P.csv_parts = r.parts;
    P.csv_names = r.names; P.csv_name_off = r.name_off;
    m6a_prep_sites_info &I = P.info;
    I.n_sites = r.NS; I.n_reads = r.R; I.n_tx = r.NT;
    I.X = r.X; I.site_kmers = r.site_kmers; I.off = r.off; I.read_prob = r.read_prob; I.site_prob = r.site_prob; I.mod_ratio = r.mod_ratio;
    I.off_host = P.off.data(); I.site_tx = P.tx.data(); I.site_pos = P.pos.data(); I.site_kmer7 = P.k7.data();
    I.tx_blob = P.blob.data(); I.tx_off = P.tx_off.data(); I.read_ids = P.ids.data();
    I.n_rep = r.n_rep; I.read_rep = P.rep.data();
}

// One file's back half: what its stages hand on, in their order.  Everything on the device is in `m`.
struct Back {
    const char *path;
    int rmin, rmax, n_threads;
    const m6a_prep_host_half *host;
    m6a_prep_sites &P;
    DevMem &m;
    Streams S;
    Fd fd;
    Front F;
    hipStream_t s = nullptr;
    double fms[6] = {0, 0, 0, 0, 0, 0}, dev_ms = 0, host_ms = 0, t1 = 0;    // t1: when the device part now running began
    int64_t NR = 0, NROW = 0;
    std::string blob;                       // this file's transcript names, in order of first appearance
    std::vector<int64_t> tx_off;
    // segments_to_host
    int64_t *sx = nullptr, *dx = nullptr, NSEG = 0, n_names = 0;
    uint8_t *dnames = nullptr;              // [n_names][16] --read_names: the file's table of names
    SegDev *seg = nullptr;
    std::vector<SegDev> hseg;
    std::vector<DeclDev> hdecl;
    // host_part
    std::vector<SegUp> up;
    std::vector<DeclUp> dup;                // the declined runs the host half combined, and their rows
    std::vector<int64_t> hpos, hrun;
    std::vector<uint8_t> hkmer;
    std::vector<double> hfeat;
    int64_t lim = 0, NT = 0, NH = 0;
    // place_runs
    RowSrc rs{};
    uint32_t *run_tx = nullptr;
    int64_t *run_place = nullptr, *dhrun = nullptr;
    uint8_t *used = nullptr;
    unsigned long long *mm = nullptr;
    // sort_rows
    uint32_t *L = nullptr, *L2 = nullptr, *row_run = nullptr;
    uint64_t *k1 = nullptr, *k2 = nullptr;
    int64_t NL = 0;
    // cut_sites
    int64_t *shx = nullptr, *start = nullptr, *kx = nullptr, *src = nullptr, *doff = nullptr, NS = 0, R = 0;
    unsigned long long *bad = nullptr;
    Back(const char *path_, int rmin_, int rmax_, const m6a_prep_host_half *host_, int n_threads_, m6a_prep_sites &P_, DevMem &m_)
        : path(path_), rmin(rmin_), rmax(rmax_), n_threads(n_threads_), host(host_), P(P_), m(m_) {}
    const char *tx_name(uint32_t t) const { return blob.data() + tx_off[t]; }
    int tx_len(uint32_t t) const { return (int)(tx_off[t + 1] - tx_off[t]); }
    int64_t seg_of(int64_t run) const       // the segment that holds the run
    {
        return (int64_t)(std::upper_bound(hseg.begin(), hseg.end(), run, [](int64_t r, const SegDev &x) { return r < x.first; }) - hseg.begin()) - 1;
    }
};

// ---- read names interned; segments and declined runs, to the host (with the name table under read_names)
int segments_to_host(Back &B)
{
    DevMem &m = B.m;
    hipStream_t s = B.s;
    const int64_t NR = B.NR;
    const bool read_names = B.P.read_names;
    int rc;
    Intern in;
    double t_in = now_ms();
    if (read_names && (rc = intern_runs(m, s, B.F.runs, B.F.rnames, NR, in))) return rc;   // from here on RunDev.read is the twin's read index
    if (read_names) B.P.ms_intern += now_ms() - t_in;
    int64_t ND = 0;
    if ((rc = m.alloc(B.sx, (size_t)NR + 1, "segments")) || (rc = m.alloc(B.dx, (size_t)NR + 1, "declined runs"))) return rc;
    if ((rc = launch(run_flags_kernel, NR, s, B.F.runs, NR, B.sx, B.dx))) return rc;
    if ((rc = read_names ? scan_total_and_names(m, B.sx, NR, s, B.NSEG, in, B.n_names) : scan_total(m, B.sx, NR, s, B.NSEG)) ||
        (rc = scan_total(m, B.dx, NR, s, ND)))
        return rc;
    if (read_names) {                                       // the table: one copy of 16 bytes per name comes to the host
        t_in = now_ms();
        if ((rc = m.alloc(B.dnames, (size_t)B.n_names * 16, "read names"))) return rc;
        if ((rc = launch(name_table_kernel, NR, s, in.val, NR, in.gx, in.rank, B.F.rnames, B.n_names, B.dnames))) return rc;
        const size_t at = B.P.names16.size();
        B.P.names16.resize(at + (size_t)B.n_names * 16);
        if ((rc = d2h(B.P.names16.data() + at, B.dnames, (size_t)B.n_names * 16, s))) return rc;
        PCHK(hipStreamSynchronize(s));
        B.P.name_off.push_back(B.P.name_off.back() + B.n_names);
        m.release({in.val, in.gx, in.rank, B.F.rnames});
        B.P.ms_intern += now_ms() - t_in;
    }
    DeclDev *decl;
    if ((rc = m.alloc(B.seg, (size_t)B.NSEG + 1, "segments")) || (rc = m.alloc(decl, (size_t)ND + 1, "declined runs"))) return rc;
    if ((rc = launch(run_lists_kernel, NR, s, B.F.runs, NR, B.sx, B.dx, B.seg, decl))) return rc;
    B.hseg.resize((size_t)B.NSEG);
    B.hdecl.resize((size_t)ND);
    if ((rc = d2h(B.hseg.data(), B.seg, (size_t)B.NSEG, s)) || (rc = d2h(B.hdecl.data(), decl, (size_t)ND, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    return M6A_OK;
}

// the transcript names of the segments (from the file where the contig changes; from the text or the saved heads where the bytes are
// on the device), every segment's transcript, the rank of its first run in it and the readcount verdict
int name_segments(Back &B)
{
    const Front &F = B.F;
    const int64_t NSEG = B.NSEG;
    int rc;
    std::vector<uint8_t> packed;                            // the contig bytes of all segments, from the device
    const bool resident = F.text || F.stream;
    if (resident) {
        std::vector<int64_t> src((size_t)NSEG), len((size_t)NSEG);
        int64_t sum = 0;                                    // a stream: the heads were saved in run order, so segment g's lie at the running sum
        for (int64_t g = 0; g < NSEG; g++) {
            src[(size_t)g] = F.stream ? sum : B.hseg[(size_t)g].contig;
            len[(size_t)g] = B.hseg[(size_t)g].len;
            sum += B.hseg[(size_t)g].len;
        }
        if (F.stream && sum != F.n_heads) return prep_fail(M6A_EHIP, "the saved contig names of %s do not add up", B.path);
        if ((rc = F.stream ? bgzf_gather(B.m, B.s, F.heads, F.n_heads, src, len, packed) : bgzf_gather(B.m, B.s, F.text, F.n, src, len, packed))) return rc;
    }
    Interner tx(B.blob, B.tx_off);
    std::vector<int64_t> tx_runs;
    std::string nm;
    B.up.resize((size_t)NSEG);
    for (int64_t g = 0, at = 0; g < NSEG; g++) {
        const SegDev &G = B.hseg[(size_t)g];
        nm.resize((size_t)G.len);
        if (resident) {
            memcpy(&nm[0], packed.data() + at, (size_t)G.len);
            at += G.len;
        } else if ((rc = read_fully(B.fd.fd, &nm[0], G.len, G.contig, B.path)))
            return rc;
        const uint32_t t = tx.id(nm);
        if (t == tx_runs.size()) tx_runs.push_back(0);
        const int64_t len = (g + 1 < NSEG ? B.hseg[(size_t)g + 1].first : B.NR) - G.first;
        B.up[(size_t)g].rank0 = tx_runs[t];
        B.up[(size_t)g].tx = t;
        tx_runs[t] += len;
    }
    B.tx_off.push_back((int64_t)B.blob.size());
    B.NT = (int64_t)tx_runs.size();
    B.lim = std::max(0, B.rmax);                            // `if ++readcount > readcount_max: break` after the first run
    for (SegUp &u : B.up) u.keep = std::min(tx_runs[u.tx], B.lim + 1) >= B.rmin;
    return M6A_OK;
}

// the declined runs the host loop reaches, combined and windowed by the host half: their npos (dup) and their rows (hpos, ...)
int host_half_rows(Back &B)
{
    const Front &F = B.F;
    int rc;
    std::vector<int64_t> cstart, cend, cread, crun;
    std::vector<int64_t> csaved;                            // a stream: where the run's bytes lie among the saved ones
    int64_t saved_at = 0;
    for (const DeclDev &d : B.hdecl) {
        const int64_t at_saved = saved_at;
        saved_at += d.end - d.start;
        const int64_t g = B.seg_of(d.run);
        if (B.up[(size_t)g].rank0 + (d.run - B.hseg[(size_t)g].first) > B.lim) continue;
        cstart.push_back(d.start); cend.push_back(d.end); cread.push_back(d.read); crun.push_back(d.run);
        csaved.push_back(at_saved);
    }
    if (F.stream && saved_at != F.n_declined) return prep_fail(M6A_EHIP, "the saved declined runs of %s do not add up", B.path);
    if (crun.empty()) return M6A_OK;
    const m6a_prep_host_half *host = B.host;
    if (!host || !host->rows || !host->table || !host->free)
        return prep_fail(M6A_EINVAL, "%zu runs need the host half and none was given", crun.size());
    struct m6a_io_rows *hr = nullptr;
    // BGZF input or a stream: the host half takes a path, so it gets the declined runs laid end to end in a plain temporary file
    struct Tmp { std::string path; ~Tmp() { if (!path.empty()) ::unlink(path.c_str()); } } tmp;
    const bool resident = F.text || F.stream;
    if (resident) {
        std::vector<uint8_t> packed;
        std::vector<int64_t> len(crun.size());
        for (size_t i = 0; i < crun.size(); i++) len[i] = cend[i] - cstart[i];
        if ((rc = F.stream ? bgzf_gather(B.m, B.s, F.declined, F.n_declined, csaved, len, packed) : bgzf_gather(B.m, B.s, F.text, F.n, cstart, len, packed)))
            return rc;
        const char *dir = getenv("TMPDIR");
        std::string name = std::string(dir && *dir ? dir : "/tmp") + "/m6a_declined_XXXXXX";
        const int tfd = ::mkstemp(&name[0]);
        if (tfd < 0) return prep_fail(M6A_EIO, "cannot create a temporary file for the declined runs of %s", B.path);
        tmp.path = name;
        rc = write_fully(tfd, packed.data(), packed.size(), name.c_str());
        ::close(tfd);
        if (rc) return rc;
        for (size_t i = 0, at = 0; i < crun.size(); i++) { cstart[i] = (int64_t)at; at += (size_t)len[i]; cend[i] = (int64_t)at; }
    }
    const int hrc = host->rows(resident ? tmp.path.c_str() : B.path, (int64_t)crun.size(), cstart.data(), cend.data(), cread.data(), 1, B.n_threads, &hr);
    if (hrc != 0 || !hr) {                                  // its own code and text (m6a_io's -1..-4 -> M6A_EINVAL, ENOMEM, EIO, EFORMAT)
        const int code = hrc == -2 ? M6A_ENOMEM : hrc == -3 ? M6A_EIO : hrc == -4 ? M6A_EFORMAT : hrc == -1 ? M6A_EINVAL : M6A_EIO;
        return prep_fail(code, "%s", host->error ? host->error() : "the host half failed on the declined runs");
    }
    struct Guard { const m6a_prep_host_half *h; struct m6a_io_rows *r; ~Guard() { h->free(r); } } guard{host, hr};
    const m6a_io_prep_table *T = host->table(hr);
    if (!T || T->n_runs != (int64_t)crun.size() || T->n_neighbors != 1) return prep_fail(M6A_EINVAL, "the host half returned a bad table");
    for (size_t i = 0; i < crun.size(); i++) {
        if (T->run_status[i] != M6A_PREP_RUN_OK) {
            const uint32_t t = B.up[(size_t)B.seg_of(crun[i])].tx;
            return prep_fail(M6A_EFORMAT, "malformed eventalign line for %.*s", B.tx_len(t), B.tx_name(t));
        }
        B.dup.push_back(DeclUp{crun[i], T->run_npos[i]});
        for (int64_t k = T->row_off[i]; k < T->row_off[i + 1]; k++) {
            B.hpos.push_back(T->row_pos[k]);
            B.hkmer.insert(B.hkmer.end(), T->row_kmer + k * 7, T->row_kmer + k * 7 + 7);
            B.hfeat.insert(B.hfeat.end(), T->row_feat + k * 9, T->row_feat + k * 9 + 9);
            B.hrun.push_back(crun[i]);
        }
    }
    return M6A_OK;
}

// ---- the host: transcript names, ranks, the readcount verdict, declined runs
// (saved_stay: the saved bytes are the caller's -- a batch of m6a_prep_group, whose later batches read on in them)
int host_part(Back &B, bool saved_stay = false)
{
    int rc;
    if ((rc = name_segments(B)) || (rc = host_half_rows(B))) return rc;
    if (!saved_stay) B.m.release({B.F.text, B.F.heads, B.F.declined});       // names and declined runs are on the host: X needs the room
    B.NH = (int64_t)B.hpos.size();
    if (B.NROW + B.NH > 0xffffffffll) return prep_fail(M6A_EINVAL, "more than 2^32 candidate rows");
    return M6A_OK;
}

// ---- runs: used or not, and their place
int place_runs(Back &B)
{
    DevMem &m = B.m;
    hipStream_t s = B.s;
    const int64_t NR = B.NR, NH = B.NH;
    RunDev *runs = B.F.runs;
    int rc;
    SegUp *dup_seg;
    DeclUp *ddecl;
    int64_t *dhpos;
    uint8_t *dhkmer;
    double *dhfeat;
    if ((rc = m.alloc(dup_seg, (size_t)B.NSEG + 1, "segments")) || (rc = m.alloc(ddecl, B.dup.size() + 1, "declined runs")) ||
        (rc = m.alloc(dhpos, (size_t)NH + 1, "host rows")) || (rc = m.alloc(B.dhrun, (size_t)NH + 1, "host rows")) ||
        (rc = m.alloc(dhkmer, (size_t)NH * 7 + 1, "host rows")) || (rc = m.alloc(dhfeat, (size_t)NH * 9 + 1, "host rows")))
        return rc;
    if ((rc = h2d(dup_seg, B.up.data(), B.up.size(), s)) || (rc = h2d(ddecl, B.dup.data(), B.dup.size(), s)) ||
        (rc = h2d(dhpos, B.hpos.data(), B.hpos.size(), s)) || (rc = h2d(B.dhrun, B.hrun.data(), B.hrun.size(), s)) ||
        (rc = h2d(dhkmer, B.hkmer.data(), B.hkmer.size(), s)) || (rc = h2d(dhfeat, B.hfeat.data(), B.hfeat.size(), s)))
        return rc;
    if ((rc = launch(decl_patch_kernel, (int64_t)B.dup.size(), s, runs, ddecl, (int64_t)B.dup.size()))) return rc;
    B.rs = RowSrc{B.F.row_pos, dhpos, B.F.row_kmer, dhkmer, B.F.row_feat, dhfeat, B.NROW};
    int64_t *run_rank, *elig, NE = 0;
    if ((rc = m.alloc(B.run_tx, (size_t)NR + 1, "runs")) || (rc = m.alloc(run_rank, (size_t)NR + 1, "runs")) || (rc = m.alloc(elig, (size_t)NR + 1, "runs")))
        return rc;
    if ((rc = launch(run_select_kernel, NR, s, runs, NR, B.sx, B.seg, dup_seg, B.lim, B.run_tx, run_rank, elig))) return rc;
    if ((rc = scan_total(m, elig, NR, s, NE))) return rc;
    uint64_t *k1, *k2;
    uint32_t *E, *E2;
    if ((rc = m.alloc(k1, (size_t)NE + 1, "runs")) || (rc = m.alloc(k2, (size_t)NE + 1, "runs")) || (rc = m.alloc(E, (size_t)NE + 1, "runs")) ||
        (rc = m.alloc(E2, (size_t)NE + 1, "runs")))
        return rc;
    unsigned long long hmm[2] = {kNone, 0};
    if ((rc = m.alloc(B.mm, 2, "flags"))) return rc;
    if ((rc = launch(compact_u32_kernel, NR, s, elig, NR, E))) return rc;
    if (NE) {
        PCHK(hipMemcpyAsync(B.mm, kMinMax0, sizeof kMinMax0, hipMemcpyHostToDevice, s));
        if ((rc = launch(minmax_kernel, NE, s, E, NE, 0, runs, B.rs, B.mm)) || (rc = d2h(hmm, B.mm, 2, s))) return rc;
        PCHK(hipStreamSynchronize(s));
        // (transcript, read): the read is the less significant
        const int bits[2] = {bits_for(hmm[1] - hmm[0]), bits_for((uint64_t)std::max<int64_t>(B.NT - 1, 0))};
        rc = sort_by_fields(m, s, bits, 2, k1, E, k2, E2, NE, [&](unsigned use, const int *shift) {
            return launch(run_key_kernel, NE, s, E, NE, runs, B.run_tx, hmm[0], shift[1], use, k1);
        });
        if (rc) return rc;
    }
    int64_t *gx, *gfirst, NG = 0;
    if ((rc = m.alloc(B.used, (size_t)NR + 1, "runs")) || (rc = m.alloc(B.run_place, (size_t)NR + 1, "runs")) || (rc = m.alloc(gx, (size_t)NE + 2, "runs")))
        return rc;
    PCHK(hipMemsetAsync(B.used, 0, (size_t)NR + 1, s));
    if ((rc = launch(dup_head_kernel, NE, s, E, NE, runs, B.run_tx, gx))) return rc;
    if ((rc = scan_total(m, gx, NE, s, NG))) return rc;
    if ((rc = m.alloc(gfirst, (size_t)NG + 1, "runs"))) return rc;
    if ((rc = launch(dup_first_kernel, NE, s, E, NE, gx, run_rank, gfirst)) || (rc = launch(dup_last_kernel, NE, s, E, NE, gx, gfirst, B.used, B.run_place)))
        return rc;
    PCHK(hipStreamSynchronize(s));
    m.release({k1, k2, E, E2, gx, gfirst, elig, B.sx, B.dx});
    return M6A_OK;
}

// ---- rows of the used runs, sorted by (transcript, position, place)
int sort_rows(Back &B)
{
    DevMem &m = B.m;
    hipStream_t s = B.s;
    const int64_t NR = B.NR, NH = B.NH;
    int rc;
    int64_t *rx, NL0 = 0, *hx, NLH = 0;
    if ((rc = m.alloc(rx, (size_t)NR + 1, "rows")) || (rc = m.alloc(hx, (size_t)NH + 1, "rows"))) return rc;
    if ((rc = launch(used_rows_count_kernel, NR, s, B.used, B.F.row_off, NR, rx))) return rc;
    if ((rc = scan_total(m, rx, NR, s, NL0))) return rc;
    if ((rc = launch(host_flag_kernel, NH, s, B.used, B.dhrun, NH, hx))) return rc;
    if ((rc = scan_total(m, hx, NH, s, NLH))) return rc;
    const int64_t NL = B.NL = NL0 + NLH;
    if ((rc = m.alloc(B.L, (size_t)NL + 1, "rows")) || (rc = m.alloc(B.L2, (size_t)NL + 1, "rows")) ||
        (rc = m.alloc(B.row_run, (size_t)(B.NROW + NH) + 1, "rows")) || (rc = m.alloc(B.k1, (size_t)NL + 1, "rows")) ||
        (rc = m.alloc(B.k2, (size_t)NL + 1, "rows")))
        return rc;
    if ((rc = launch(used_rows_write_kernel, NR, s, B.used, B.F.row_off, NR, rx, B.L, B.row_run)) ||
        (rc = launch(host_rows_kernel, NH, s, B.dhrun, NH, B.NROW, NL0, hx, B.L, B.row_run)))
        return rc;
    if (!NL) return M6A_OK;
    unsigned long long hmm[2] = {kNone, 0};
    PCHK(hipMemcpyAsync(B.mm, kMinMax0, sizeof kMinMax0, hipMemcpyHostToDevice, s));
    if ((rc = launch(minmax_kernel, NL, s, B.L, NL, 1, B.F.runs, B.rs, B.mm)) || (rc = d2h(hmm, B.mm, 2, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    // place, position, transcript: least significant first
    const int bits[3] = {bits_for((uint64_t)B.lim), bits_for(hmm[1] - hmm[0]), bits_for((uint64_t)std::max<int64_t>(B.NT - 1, 0))};
    return sort_by_fields(m, s, bits, 3, B.k1, B.L, B.k2, B.L2, NL, [&](unsigned use, const int *shift) {
        const RowKey key{hmm[0], shift[2], shift[1], shift[0], (use & 4 ? 1u : 0u) | (use & 2) | (use & 1 ? 4u : 0u)};
        return launch(row_key_kernel, NL, s, B.L, NL, B.rs, B.row_run, B.run_tx, B.run_place, key, B.k1);
    });
}

// ---- sites: cut, checked, filtered -- kept with at least `need` reads
int cut_sites(Back &B, int64_t need)
{
    DevMem &m = B.m;
    hipStream_t s = B.s;
    const int64_t NL = B.NL;
    int rc;
    int64_t NS0 = 0;
    if ((rc = m.alloc(B.shx, (size_t)NL + 1, "sites"))) return rc;
    if ((rc = launch(site_head_kernel, NL, s, B.L, NL, B.rs, B.row_run, B.run_tx, B.shx))) return rc;
    if ((rc = scan_total(m, B.shx, NL, s, NS0))) return rc;
    unsigned long long hbad = kNone;
    if ((rc = m.alloc(B.start, (size_t)NS0 + 1, "sites")) || (rc = m.alloc(B.kx, (size_t)NS0 + 1, "sites")) || (rc = m.alloc(B.bad, 1, "flags"))) return rc;
    PCHK(hipMemcpyAsync(B.bad, &kNone, sizeof kNone, hipMemcpyHostToDevice, s));
    if ((rc = launch(site_start_kernel, NL, s, B.shx, NL, B.start)) || (rc = launch(site_check_kernel, NL, s, B.L, NL, B.rs, B.shx, B.start, B.bad)))
        return rc;
    if ((rc = fetch(hbad, B.bad, s))) return rc;
    if (hbad != ~0ull) {
        int64_t *probe, hp[2] = {0, 0};
        if ((rc = m.alloc(probe, 2, "flags"))) return rc;
        probe_kernel<<<1, 1, 0, s>>>(B.L, B.start, (int64_t)hbad, B.rs, B.row_run, B.run_tx, probe);
        PCHK(hipGetLastError());
        if ((rc = d2h(hp, probe, 2, s))) return rc;
        PCHK(hipStreamSynchronize(s));
        return prep_fail(M6A_EFORMAT, "reads disagree on the sequence at %.*s:%lld", B.tx_len((uint32_t)hp[0]), B.tx_name((uint32_t)hp[0]), (long long)hp[1]);
    }
    if ((rc = launch(site_keep_kernel, NS0, s, B.start, NS0, need, B.kx))) return rc;
    if ((rc = scan_total(m, B.kx, NS0, s, B.NS))) return rc;
    if ((rc = m.alloc(B.src, (size_t)B.NS + 1, "sites")) || (rc = m.alloc(B.doff, (size_t)B.NS + 1, "the offsets"))) return rc;
    PCHK(hipMemsetAsync(B.doff + B.NS, 0, sizeof(int64_t), s));
    if ((rc = launch(site_emit_kernel, NS0, s, B.start, NS0, B.kx, B.src, B.doff))) return rc;
    return scan_total(m, B.doff, B.NS, s, B.R);
}

// dataprep: no normalisation, no vocabulary, and text instead of X
int finish_dataprep(Back &B, const DataprepJob &job)
{
    DevMem &m = B.m;
    hipStream_t s = B.s;
    const int64_t NS = B.NS;
    int rc;
    uint32_t *jtx;
    int64_t *jpos;
    uint8_t *jk7, *jkm;
    int32_t *jnorm;
    if ((rc = m.alloc(jtx, (size_t)NS + 1, "sites")) || (rc = m.alloc(jpos, (size_t)NS + 1, "sites")) || (rc = m.alloc(jk7, (size_t)NS * 7 + 1, "sites")) ||
        (rc = m.alloc(jkm, (size_t)NS * 3 + 1, "sites")) || (rc = m.alloc(jnorm, (size_t)NS * 3 + 1, "sites")))
        return rc;
    if ((rc = launch(site_info_kernel, NS, s, B.L, B.src, NS, B.rs, B.row_run, B.run_tx, nullptr, nullptr, 0, nullptr, 0, jnorm, jkm, jtx, jpos, jk7,
                     B.bad, nullptr, 1)))
        return rc;
    PCHK(hipStreamSynchronize(s));
    m.release({jkm, jnorm, B.k1, B.k2, B.L2, B.shx, B.start, B.kx});
    B.dev_ms += now_ms() - B.t1;
    job.st->ms_front = B.fms[0] + B.fms[1] + B.fms[2];
    job.st->ms_back = B.dev_ms + B.host_ms;
    const DataprepSrc ds{JsonDev{B.L, B.src, B.doff, B.rs, B.row_run, B.F.runs, jtx, jpos, jk7, nullptr, nullptr, 0}, B.run_tx, NS, B.NR, B.NL, B.NT,
                         &B.blob, &B.tx_off};
    return dataprep_emit(m, s, job, ds);
}

// normalisation and vocabulary of the kept sites (site_info_kernel), for finish_part and finish_single
struct SiteInfo {
    int32_t *site_norm;
    double *dmean, *dstd;
    uint32_t *site_tx;
    int64_t *site_pos;
    uint8_t *site_k7, *site_kmers;
};

// tx_map (one replicate of several): this file's transcript ids -> the job's, and the checks wait for the pooled sites
int site_info(Back &B, const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm, const std::vector<uint32_t> *tx_map, SiteInfo &I)
{
    DevMem &m = B.m;
    hipStream_t s = B.s;
    const int64_t NS = B.NS;
    int rc;
    std::vector<uint64_t> nk, voc = vocab_keys();
    std::vector<int32_t> nix;
    norm_keys(norm_kmers, n_norm, nk, nix);
    uint64_t *dnk, *dvoc;
    int32_t *dnix;
    if ((rc = m.alloc(dnk, nk.size() + 1, "norm")) || (rc = m.alloc(dnix, nix.size() + 1, "norm")) || (rc = m.alloc(dvoc, voc.size(), "norm")) ||
        (rc = m.alloc(I.dmean, (size_t)n_norm * 3 + 1, "norm")) || (rc = m.alloc(I.dstd, (size_t)n_norm * 3 + 1, "norm")) ||
        (rc = m.alloc(I.site_norm, (size_t)NS * 3 + 1, "sites")) || (rc = m.alloc(I.site_tx, (size_t)NS + 1, "sites")) ||
        (rc = m.alloc(I.site_pos, (size_t)NS + 1, "sites")) || (rc = m.alloc(I.site_k7, (size_t)NS * 7 + 1, "sites")) ||
        (rc = m.alloc(I.site_kmers, (size_t)NS * 3 + 1, "site k-mers")))
        return rc;
    uint32_t *dmap = nullptr;
    if (tx_map && ((rc = m.alloc(dmap, tx_map->size() + 1, "transcripts")) || (rc = h2d(dmap, tx_map->data(), tx_map->size(), s)))) return rc;
    if ((rc = h2d(dnk, nk.data(), nk.size(), s)) || (rc = h2d(dnix, nix.data(), nix.size(), s)) || (rc = h2d(dvoc, voc.data(), voc.size(), s)) ||
        (rc = h2d(I.dmean, norm_mean, (size_t)n_norm * 3, s)) || (rc = h2d(I.dstd, norm_std, (size_t)n_norm * 3, s)))
        return rc;
    PCHK(hipMemcpyAsync(B.bad, &kNone, sizeof kNone, hipMemcpyHostToDevice, s));
    return launch(site_info_kernel, NS, s, B.L, B.src, NS, B.rs, B.row_run, B.run_tx, dnk, dnix, (int)nk.size(), dvoc, (int)voc.size(), I.site_norm,
                  I.site_kmers, I.site_tx, I.site_pos, I.site_k7, B.bad, dmap, tx_map ? 1 : 0);
}

// one replicate of several: X per candidate read, and what pool_impl needs of the sites, stay as a FilePart; the rest of the file goes
int finish_part(Back &B, Pool &pool, size_t mark, const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm)
{
    DevMem &m = B.m;
    hipStream_t s = B.s;
    int rc;
    std::vector<uint32_t> l2g;                              // this file's transcript ids -> the job's
    for (int64_t t = 0; t < B.NT; t++) l2g.push_back(pool.tx.id(std::string(B.tx_name((uint32_t)t), (size_t)B.tx_len((uint32_t)t))));
    SiteInfo I;
    if ((rc = site_info(B, norm_kmers, norm_mean, norm_std, n_norm, &l2g, I))) return rc;
    if (B.R > 0x7fffffffll) return prep_fail(M6A_EINVAL, "more than 2^31 candidate reads in %s", B.path);
    FilePart fp;
    if ((rc = m.alloc(fp.X, (size_t)B.R * 9, "X")) || (rc = m.alloc(fp.ids, (size_t)B.R + 1, "read ids"))) return rc;
    if ((rc = launch(x_kernel, B.R, s, B.L, B.src, B.doff, B.NS, B.R, B.rs, B.row_run, B.F.runs, I.site_norm, I.dmean, I.dstd, n_norm, fp.X, fp.ids)))
        return rc;
    PCHK(hipStreamSynchronize(s));
    fp.NC = B.NS; fp.RC = B.R; fp.tx = I.site_tx; fp.pos = I.site_pos; fp.k7 = I.site_k7; fp.off = B.doff;
    fp.names = B.dnames; fp.n_names = B.n_names;
    m.release_since(mark, {fp.X, fp.ids, fp.tx, fp.pos, fp.k7, fp.off, fp.names});
    pool.parts.push_back(fp);
    B.dev_ms += now_ms() - B.t1;
    return M6A_OK;
}

// the whole job (m6a_prep_sites_build): P filled
int finish_single(Back &B, const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm, double *ms)
{
    DevMem &m = B.m;
    hipStream_t s = B.s;
    m6a_prep_sites &P = B.P;
    const int64_t NS = B.NS, R = B.R;
    int rc;
    P.blob.swap(B.blob);                                    // the file's names are the job's
    P.tx_off.swap(B.tx_off);
    SiteInfo I;
    if ((rc = site_info(B, norm_kmers, norm_mean, norm_std, n_norm, nullptr, I))) return rc;
    P.off.resize((size_t)NS + 1); P.tx.resize((size_t)NS); P.pos.resize((size_t)NS); P.k7.resize((size_t)NS * 7);
    unsigned long long hbad = kNone;
    if ((rc = d2h(&hbad, B.bad, 1, s)) || (rc = d2h(P.off.data(), B.doff, (size_t)NS + 1, s)) || (rc = d2h(P.tx.data(), I.site_tx, (size_t)NS, s)) ||
        (rc = d2h(P.pos.data(), I.site_pos, (size_t)NS, s)) || (rc = d2h((uint8_t *)P.k7.data(), I.site_k7, (size_t)NS * 7, s)))
        return rc;
    PCHK(hipStreamSynchronize(s));
    if (hbad != ~0ull) return bad_site(P, hbad, false);
    float *X;
    double *dids;
    if ((rc = m.alloc(X, (size_t)R * 9, "X")) || (rc = m.alloc(dids, (size_t)R + 1, "read ids"))) return rc;
    if ((rc = launch(x_kernel, R, s, B.L, B.src, B.doff, NS, R, B.rs, B.row_run, B.F.runs, I.site_norm, I.dmean, I.dstd, n_norm, X, dids))) return rc;
    P.ids.resize((size_t)R);
    PCHK(hipStreamSynchronize(s));
    B.dev_ms += now_ms() - B.t1;
    const double t1 = now_ms();
    if ((rc = d2h(P.ids.data(), dids, (size_t)R, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    ms[5] = now_ms() - t1;
    float *rp, *sp;
    double *mr;
    if ((rc = m.alloc(rp, (size_t)R, "read probabilities")) || (rc = m.alloc(sp, (size_t)NS, "site probabilities")) ||
        (rc = m.alloc(mr, (size_t)NS, "mod ratios")))
        return rc;
    int64_t *dname_off = nullptr;
    if (P.read_names) {
        if ((rc = m.alloc(dname_off, 2, "read names")) || (rc = h2d(dname_off, P.name_off.data(), 2, s))) return rc;
        PCHK(hipStreamSynchronize(s));
    }
    P.rep.assign((size_t)R, 0);
    publish(P, m, Result{NS, R, B.NT, 1, X, I.site_kmers, B.doff, rp, sp, mr, I.site_tx, I.site_pos, I.site_k7, dids, nullptr, B.dnames, dname_off});
    return M6A_OK;
}

// One file.  pool == nullptr and job == nullptr: the whole job (m6a_prep_sites_build), P filled.  pool: the file is one replicate of
// several -- its sites with >= min_seg reads (the 20-read floor and the per-site checks wait for the pooled sites, pool_impl), their X
// and read ids stay on the device as a FilePart, and everything else the file needed -- its text, line records, candidate rows -- is
// released.  job: `dataprep --writer device` (m6a_dataprep.h).
int sites_impl(int device_id, const char *path, int rmin, int rmax, int min_seg, const char *norm_kmers, const double *norm_mean,
               const double *norm_std, int n_norm, const m6a_prep_host_half *host, int n_threads, int64_t window, m6a_prep_sites &P, DevMem &m,
               double *ms, Pool *pool, const DataprepJob *job = nullptr)
{
    const double t_all = now_ms();
    const size_t mark = m.ptrs.size();
    Back B(path, rmin, rmax, host, n_threads, P, m);
    Front &F = B.F;
    F.bgzf_ok = !job;                                       // dataprep's index holds offsets into the text: BGZF and streams stay refused
    F.read_names = P.read_names;
    int rc = front_half(device_id, path, 1, nullptr, nullptr, window, m, B.S, B.fd, F, B.fms);
    if (rc) return rc;
    P.info.n_bgzf_blocks += F.n_blocks;
    P.info.compressed_bytes += F.comp_bytes;
    P.info.ms_inflate += F.ms_inflate;
    P.info.n_windows += F.n_windows;
    P.info.window_bytes = std::max(P.info.window_bytes, F.window_bytes);
    if (F.stream) { P.stream_bytes += F.n; P.n_streams += 1; }
    ms[0] = B.fms[0]; ms[1] = B.fms[1]; ms[2] = B.fms[2]; ms[6] = B.fms[5];
    B.s = B.S.s[0];
    PCHK(hipStreamSynchronize(B.s));
    for (const void *p : F.scratch) m.release(p);          // the file and its line records: X needs the room
    B.NR = F.NR; B.NROW = F.NROW;
    if (B.NR > 0xffffffffll) return prep_fail(M6A_EINVAL, "more than 2^32 runs");

    B.t1 = now_ms();
    if ((rc = segments_to_host(B))) return rc;
    B.dev_ms += now_ms() - B.t1;
    B.t1 = now_ms();
    if ((rc = host_part(B))) return rc;
    B.host_ms += now_ms() - B.t1;
    B.t1 = now_ms();                                        // the finishes close this interval
    if ((rc = place_runs(B)) || (rc = sort_rows(B)) || (rc = cut_sites(B, pool || job ? (int64_t)min_seg : std::max<int64_t>(min_seg, 20)))) return rc;
    if (job) return finish_dataprep(B, *job);
    if ((rc = pool ? finish_part(B, *pool, mark, norm_kmers, norm_mean, norm_std, n_norm) : finish_single(B, norm_kmers, norm_mean, norm_std, n_norm, ms)))
        return rc;
    ms[3] = B.dev_ms; ms[4] = B.host_ms; ms[7] = now_ms() - t_all;
    return M6A_OK;
}


// ---- replicates (m6a_prep_sites_build_multi): the union of the files' sites, formed where the features are ------------------------
// Every file leaves a FilePart.  Their sites, numbered file after file ("candidates"), are keyed by (transcript, position):
//   groups     one stable sort of the candidate numbers by the key: a group = the parts of one pooled site, in file order
//   order      a group's first member is where the site first appears; an exclusive scan of those flags over the candidates, in
//              their own order, numbers the pooled sites -- file 0's sites in file 0's order, then what file 1 adds, ...
//   filter     reads summed over the parts; kept with >= 20; scan -> off; per (kept site, file) the block of rows it supplies
//   checks     kept sites only, lowest first (atomicMin): the first part's normalisation factors, later parts' 7-mers against the
//              first, the vocabulary -- m6a_io_load_sites' order
//   copy       a wave per (kept site, file): the block's 9 n dwords of X and n read ids, lane after lane
constexpr int64_t kMinReads = 20;          // DEFAULT_MIN_READS: the loader's floor on the pooled count

__global__ void cand_fill_kernel(const int64_t *__restrict__ off, int64_t n, int64_t base, int32_t file, int64_t *__restrict__ c_src,
                                 int32_t *__restrict__ c_cnt, int32_t *__restrict__ c_file, uint32_t *__restrict__ val)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    c_src[base + i] = off[i];
    c_cnt[base + i] = (int32_t)(off[i + 1] - off[i]);
    c_file[base + i] = file;
    val[base + i] = (uint32_t)(base + i);
}

__global__ void cand_minmax_kernel(const int64_t *__restrict__ pos, int64_t n, unsigned long long *__restrict__ mm)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    unsigned long long lo = ~0ull, hi = 0;
    if (i < n) lo = hi = bias(pos[i]);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) { atomicMin(&mm[0], lo); atomicMax(&mm[1], hi); }
}

// use: 1 = the position part, 2 = the transcript part (shifted by tx_shift)
__global__ void cand_key_kernel(const uint32_t *__restrict__ val, int64_t n, const uint32_t *__restrict__ c_tx, const int64_t *__restrict__ c_pos,
                                uint64_t pos_min, int tx_shift, unsigned use, uint64_t *__restrict__ key)
{
    const int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = val[j];
    uint64_t v = 0;
    if (use & 1) v |= bias(c_pos[i]) - pos_min;
    if (use & 2) v |= (uint64_t)c_tx[i] << tx_shift;
    key[j] = v;
}

__global__ void cand_head_kernel(const uint32_t *__restrict__ val, int64_t n, const uint32_t *__restrict__ c_tx, const int64_t *__restrict__ c_pos,
                                 int64_t *__restrict__ head)
{
    const int64_t j = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (j >= n) return;
    head[j] = j == 0 || c_tx[val[j]] != c_tx[val[j - 1]] || c_pos[val[j]] != c_pos[val[j - 1]];
}

__global__ void group_first_kernel(const uint32_t *__restrict__ val, const int64_t *__restrict__ gstart, int64_t NG, int64_t *__restrict__ first)
{
    const int64_t g = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (g < NG) first[val[gstart[g]]] = 1;
}

// per group: its pooled number u (before the filter), its reads summed, kept or not
__global__ void group_sum_kernel(const uint32_t *__restrict__ val, const int64_t *__restrict__ gstart, int64_t NG, const int32_t *__restrict__ c_cnt,
                                 const int64_t *__restrict__ ux, int64_t *__restrict__ usum, int64_t *__restrict__ ugrp, int64_t *__restrict__ keep)
{
    const int64_t g = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (g >= NG) return;
    int64_t sum = 0;
    for (int64_t j = gstart[g]; j < gstart[g + 1]; j++) sum += c_cnt[val[j]];
    const int64_t u = ux[val[gstart[g]]];
    usum[u] = sum;
    ugrp[u] = g;
    keep[u] = sum >= kMinReads;
}

__global__ void pool_emit_kernel(const int64_t *__restrict__ kx, int64_t NG, const int64_t *__restrict__ usum, const int64_t *__restrict__ ugrp,
                                 int64_t *__restrict__ off, int64_t *__restrict__ kgrp)
{
    const int64_t u = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (u >= NG || kx[u + 1] == kx[u]) return;
    off[kx[u]] = usum[u];
    kgrp[kx[u]] = ugrp[u];
}

// per kept site: transcript, position and 7-mer of its first part; per part the block it supplies (blk_* [S][K], by file; a file
// holds a (transcript, position) once, so a group has at most one member per file); then the checks; bad = 8 site + what
// (0..2 a 5-mer without normalisation factors, 3 a later part's 7-mer differs, 4..6 a 5-mer outside the vocabulary)
__global__ void pool_site_kernel(const uint32_t *__restrict__ val, const int64_t *__restrict__ gstart, const int64_t *__restrict__ kgrp, int64_t S, int K,
                                 const int64_t *__restrict__ off, const uint32_t *__restrict__ c_tx, const int64_t *__restrict__ c_pos,
                                 const uint8_t *__restrict__ c_k7, const int64_t *__restrict__ c_src, const int32_t *__restrict__ c_cnt,
                                 const int32_t *__restrict__ c_file, const uint64_t *__restrict__ nkeys, int n_norm, const uint64_t *__restrict__ vocab,
                                 int n_vocab, uint32_t *__restrict__ site_tx, int64_t *__restrict__ site_pos, uint8_t *__restrict__ site_k7,
                                 uint8_t *__restrict__ site_kmers, int64_t *__restrict__ blk_src, int64_t *__restrict__ blk_dst,
                                 int32_t *__restrict__ blk_cnt, unsigned long long *__restrict__ bad)
{
    const int64_t s = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (s >= S) return;
    const int64_t g = kgrp[s], j0 = gstart[g], j1 = gstart[g + 1];
    const uint32_t i0 = val[j0];
    const uint8_t *km = c_k7 + (int64_t)i0 * 7;
    site_tx[s] = c_tx[i0];
    site_pos[s] = c_pos[i0];
    for (int c = 0; c < 7; c++) site_k7[s * 7 + c] = km[c];
    int64_t row = off[s];
    bool differ = false;
    for (int64_t j = j0; j < j1; j++) {
        const uint32_t i = val[j];
        const int64_t b = s * K + c_file[i];
        blk_src[b] = c_src[i];
        blk_dst[b] = row;
        blk_cnt[b] = c_cnt[i];
        row += c_cnt[i];
        for (int c = 0; c < 7; c++) differ |= c_k7[(int64_t)i * 7 + c] != km[c];
    }
    for (int c = 0; c < 3 && n_norm; c++)
        if (find5(nkeys, n_norm, pack5(km + c)) < 0) { atomicMin(bad, (unsigned long long)(s * 8 + c)); return; }
    if (differ) { atomicMin(bad, (unsigned long long)(s * 8 + 3)); return; }
    for (int c = 0; c < 3; c++) {
        const int v = find5(vocab, n_vocab, pack5(km + c));
        if (v < 0) { atomicMin(bad, (unsigned long long)(s * 8 + 4 + c)); return; }
        site_kmers[s * 3 + c] = (uint8_t)v;
    }
}

// a wave per (kept site, file): its block of n rows is 36 n bytes of X and 8 n of read ids, contiguous on both sides and 4-byte
// aligned (rows are 36 B), so consecutive lanes move consecutive dwords; an empty block ends at once
__global__ void pool_copy_kernel(int64_t n_blocks, int K, const int64_t *__restrict__ blk_src, const int64_t *__restrict__ blk_dst,
                                 const int32_t *__restrict__ blk_cnt, const float *const *__restrict__ Xs, const double *const *__restrict__ ids_s,
                                 float *__restrict__ X, double *__restrict__ ids)
{
    const int64_t b = (int64_t)blockIdx.x * (kBlk / 64) + (threadIdx.x >> 6);
    if (b >= n_blocks) return;
    const int64_t n = blk_cnt[b];
    if (n == 0) return;
    const int f = (int)(b % K), lane = threadIdx.x & 63;
    const uint32_t *src = (const uint32_t *)Xs[f] + blk_src[b] * 9;
    uint32_t *dst = (uint32_t *)X + blk_dst[b] * 9;
    for (int64_t d = lane; d < n * 9; d += 64) dst[d] = src[d];
    const double *isrc = ids_s[f] + blk_src[b];
    double *idst = ids + blk_dst[b];
    for (int64_t d = lane; d < n; d += 64) idst[d] = isrc[d];
}

int pool_impl(Pool &pool, const char *norm_kmers, int n_norm, DevMem &m, m6a_prep_sites &P, double *ms)
{
    double t1 = now_ms();
    Streams S;
    PCHK(hipStreamCreateWithFlags(&S.s[0], hipStreamNonBlocking));
    hipStream_t s = S.s[0];
    const int K = (int)pool.parts.size();
    int64_t NC = 0;
    for (const FilePart &fp : pool.parts) NC += fp.NC;
    if (NC > 0xffffffffll) return prep_fail(M6A_EINVAL, "more than 2^32 candidate sites");
    const int64_t NT = (int64_t)pool.tx.ids.size();
    P.tx_off.push_back((int64_t)P.blob.size());
    int rc;

    // ---- the candidates of all files, file after file
    uint32_t *c_tx, *val, *val2;
    int64_t *c_pos, *c_src;
    int32_t *c_cnt, *c_file;
    uint8_t *c_k7;
    uint64_t *k1, *k2;
    if ((rc = m.alloc(c_tx, (size_t)NC + 1, "pooled sites")) || (rc = m.alloc(c_pos, (size_t)NC + 1, "pooled sites")) ||
        (rc = m.alloc(c_src, (size_t)NC + 1, "pooled sites")) || (rc = m.alloc(c_cnt, (size_t)NC + 1, "pooled sites")) ||
        (rc = m.alloc(c_file, (size_t)NC + 1, "pooled sites")) || (rc = m.alloc(c_k7, (size_t)NC * 7 + 1, "pooled sites")) ||
        (rc = m.alloc(val, (size_t)NC + 1, "pooled sites")) || (rc = m.alloc(val2, (size_t)NC + 1, "pooled sites")) ||
        (rc = m.alloc(k1, (size_t)NC + 1, "pooled sites")) || (rc = m.alloc(k2, (size_t)NC + 1, "pooled sites")))
        return rc;
    int64_t base = 0;
    for (int f = 0; f < K; f++) {
        const FilePart &fp = pool.parts[(size_t)f];
        if (!fp.NC) continue;
        PCHK(hipMemcpyAsync(c_tx + base, fp.tx, (size_t)fp.NC * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        PCHK(hipMemcpyAsync(c_pos + base, fp.pos, (size_t)fp.NC * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        PCHK(hipMemcpyAsync(c_k7 + base * 7, fp.k7, (size_t)fp.NC * 7, hipMemcpyDeviceToDevice, s));
        if ((rc = launch(cand_fill_kernel, fp.NC, s, fp.off, fp.NC, base, f, c_src, c_cnt, c_file, val))) return rc;
        base += fp.NC;
    }
    PCHK(hipStreamSynchronize(s));
    for (FilePart &fp : pool.parts) {
        m.release({fp.tx, fp.pos, fp.k7, fp.off});
        fp.tx = nullptr; fp.pos = fp.off = nullptr; fp.k7 = nullptr;
    }

    // ---- groups: the candidates sorted by (transcript, position), stable, so that a group's members are in file order
    unsigned long long *mm, hmm[2] = {kNone, 0};
    if ((rc = m.alloc(mm, 2, "flags"))) return rc;
    if (NC) {
        PCHK(hipMemcpyAsync(mm, kMinMax0, sizeof kMinMax0, hipMemcpyHostToDevice, s));
        if ((rc = launch(cand_minmax_kernel, NC, s, c_pos, NC, mm)) || (rc = d2h(hmm, mm, 2, s))) return rc;
        PCHK(hipStreamSynchronize(s));
        // (transcript, position): the position is the less significant
        const int bits[2] = {bits_for(hmm[1] - hmm[0]), bits_for((uint64_t)std::max<int64_t>(NT - 1, 0))};
        rc = sort_by_fields(m, s, bits, 2, k1, val, k2, val2, NC, [&](unsigned use, const int *shift) {
            return launch(cand_key_kernel, NC, s, val, NC, c_tx, c_pos, hmm[0], shift[1], use, k1);
        });
        if (rc) return rc;
    }
    int64_t *gx, *gstart, *ux, NG = 0, NU = 0;
    if ((rc = m.alloc(gx, (size_t)NC + 1, "pooled sites")) || (rc = m.alloc(ux, (size_t)NC + 1, "pooled sites"))) return rc;
    if ((rc = launch(cand_head_kernel, NC, s, val, NC, c_tx, c_pos, gx))) return rc;
    if ((rc = scan_total(m, gx, NC, s, NG))) return rc;
    if ((rc = m.alloc(gstart, (size_t)NG + 1, "pooled sites"))) return rc;
    PCHK(hipMemsetAsync(ux, 0, (size_t)(NC + 1) * sizeof(int64_t), s));
    if ((rc = launch(site_start_kernel, NC, s, gx, NC, gstart)) || (rc = launch(group_first_kernel, NG, s, val, gstart, NG, ux))) return rc;
    if ((rc = scan_total(m, ux, NC, s, NU))) return rc;
    if (NU != NG) return prep_fail(M6A_EINVAL, "pooled sites: %lld groups, %lld first members", (long long)NG, (long long)NU);

    // ---- the pooled filter and the offsets
    int64_t *usum, *ugrp, *kx, *kgrp, *doff, NS = 0, R = 0;
    if ((rc = m.alloc(usum, (size_t)NG + 1, "pooled sites")) || (rc = m.alloc(ugrp, (size_t)NG + 1, "pooled sites")) ||
        (rc = m.alloc(kx, (size_t)NG + 1, "pooled sites")))
        return rc;
    if ((rc = launch(group_sum_kernel, NG, s, val, gstart, NG, c_cnt, ux, usum, ugrp, kx))) return rc;
    if ((rc = scan_total(m, kx, NG, s, NS))) return rc;
    if ((rc = m.alloc(kgrp, (size_t)NS + 1, "pooled sites")) || (rc = m.alloc(doff, (size_t)NS + 1, "the offsets"))) return rc;
    if ((rc = launch(pool_emit_kernel, NG, s, kx, NG, usum, ugrp, doff, kgrp))) return rc;
    if ((rc = scan_total(m, doff, NS, s, R))) return rc;

    // ---- per kept site: its arrays, its blocks, its checks
    std::vector<uint64_t> nk, voc = vocab_keys();
    std::vector<int32_t> nix;                               // not needed here: the files' X is normalised already
    norm_keys(norm_kmers, n_norm, nk, nix);
    uint64_t *dnk, *dvoc;
    uint32_t *site_tx;
    int64_t *site_pos, *blk_src, *blk_dst;
    int32_t *blk_cnt;
    uint8_t *site_k7, *site_kmers;
    unsigned long long *bad, hbad = kNone;
    const size_t NB = (size_t)NS * (size_t)K;
    if ((rc = m.alloc(dnk, nk.size() + 1, "norm")) || (rc = m.alloc(dvoc, voc.size(), "norm")) || (rc = m.alloc(site_tx, (size_t)NS + 1, "sites")) ||
        (rc = m.alloc(site_pos, (size_t)NS + 1, "sites")) || (rc = m.alloc(site_k7, (size_t)NS * 7 + 1, "sites")) ||
        (rc = m.alloc(site_kmers, (size_t)NS * 3 + 1, "site k-mers")) || (rc = m.alloc(blk_src, NB + 1, "blocks")) ||
        (rc = m.alloc(blk_dst, NB + 1, "blocks")) || (rc = m.alloc(blk_cnt, NB + 1, "blocks")) || (rc = m.alloc(bad, 1, "flags")))
        return rc;
    if ((rc = h2d(dnk, nk.data(), nk.size(), s)) || (rc = h2d(dvoc, voc.data(), voc.size(), s))) return rc;
    PCHK(hipMemcpyAsync(bad, &kNone, sizeof kNone, hipMemcpyHostToDevice, s));
    PCHK(hipMemsetAsync(blk_cnt, 0, (NB + 1) * sizeof(int32_t), s));
    PCHK(hipMemsetAsync(blk_src, 0, (NB + 1) * sizeof(int64_t), s));
    PCHK(hipMemsetAsync(blk_dst, 0, (NB + 1) * sizeof(int64_t), s));
    if ((rc = launch(pool_site_kernel, NS, s, val, gstart, kgrp, NS, K, doff, c_tx, c_pos, c_k7, c_src, c_cnt, c_file, dnk, (int)nk.size(), dvoc,
                     (int)voc.size(), site_tx, site_pos, site_k7, site_kmers, blk_src, blk_dst, blk_cnt, bad)))
        return rc;
    P.off.resize((size_t)NS + 1);
    P.tx.resize((size_t)NS);
    P.pos.resize((size_t)NS);
    P.k7.resize((size_t)NS * 7);
    std::vector<int32_t> cnt(NB);
    if ((rc = d2h(&hbad, bad, 1, s)) || (rc = d2h(P.off.data(), doff, (size_t)NS + 1, s)) || (rc = d2h(P.tx.data(), site_tx, (size_t)NS, s)) ||
        (rc = d2h(P.pos.data(), site_pos, (size_t)NS, s)) || (rc = d2h((uint8_t *)P.k7.data(), site_k7, (size_t)NS * 7, s)) ||
        (rc = d2h(cnt.data(), blk_cnt, NB, s)))
        return rc;
    PCHK(hipStreamSynchronize(s));
    if (hbad != ~0ull) return bad_site(P, hbad, true);

    // ---- the pooled X and read ids
    float *X;
    double *dids;
    const float **dXs;
    const double **dis;
    if ((rc = m.alloc(X, (size_t)R * 9, "X")) || (rc = m.alloc(dids, (size_t)R + 1, "read ids")) || (rc = m.alloc(dXs, (size_t)K, "blocks")) ||
        (rc = m.alloc(dis, (size_t)K, "blocks")))
        return rc;
    std::vector<const float *> hXs;
    std::vector<const double *> his;
    for (const FilePart &fp : pool.parts) { hXs.push_back(fp.X); his.push_back(fp.ids); }
    if ((rc = h2d(dXs, hXs.data(), hXs.size(), s)) || (rc = h2d(dis, his.data(), his.size(), s))) return rc;
    if (NB && R) {
        const int64_t nblk = ((int64_t)NB + kBlk / 64 - 1) / (kBlk / 64);
        if (nblk > 0x7fffffffll) return prep_fail(M6A_EINVAL, "more than 2^33 (site, replicate) blocks");
        pool_copy_kernel<<<(unsigned)nblk, kBlk, 0, s>>>((int64_t)NB, K, blk_src, blk_dst, blk_cnt, dXs, dis, X, dids);
        PCHK(hipGetLastError());
    }
    P.rep.resize((size_t)R);
    for (int64_t i = 0, r = 0; i < NS; i++)
        for (int f = 0; f < K; f++)
            for (int32_t k = 0; k < cnt[(size_t)(i * K + f)]; k++) P.rep[(size_t)r++] = f;
    P.ids.resize((size_t)R);
    PCHK(hipStreamSynchronize(s));
    ms[3] += now_ms() - t1;
    t1 = now_ms();
    if ((rc = d2h(P.ids.data(), dids, (size_t)R, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    ms[5] += now_ms() - t1;
    float *rp, *sp;
    double *mr;
    if ((rc = m.alloc(rp, (size_t)R, "read probabilities")) || (rc = m.alloc(sp, (size_t)NS, "site probabilities")) ||
        (rc = m.alloc(mr, (size_t)NS, "mod ratios")))
        return rc;
    uint8_t *dnames = nullptr;
    int64_t *dname_off = nullptr;
    if (P.read_names) {                                     // the files' tables, one behind the other
        if ((rc = m.alloc(dnames, P.names16.size(), "read names")) || (rc = m.alloc(dname_off, P.name_off.size(), "read names")) ||
            (rc = h2d(dname_off, P.name_off.data(), P.name_off.size(), s)))
            return rc;
        for (int f = 0; f < K; f++)
            if (pool.parts[(size_t)f].n_names)
                PCHK(hipMemcpyAsync(dnames + P.name_off[(size_t)f] * 16, pool.parts[(size_t)f].names, (size_t)pool.parts[(size_t)f].n_names * 16,
                                    hipMemcpyDeviceToDevice, s));
        PCHK(hipStreamSynchronize(s));
        for (FilePart &fp : pool.parts) { m.release(fp.names); fp.names = nullptr; }
    }
    publish(P, m, Result{NS, R, NT, K, X, site_kmers, doff, rp, sp, mr, site_tx, site_pos, site_k7, dids, blk_cnt, dnames, dname_off});
    return M6A_OK;
}

int sites_multi(int device_id, const char *const *paths, int n_paths, int rmin, int rmax, int min_seg, const char *norm_kmers,
                const double *norm_mean, const double *norm_std, int n_norm, const m6a_prep_host_half *host, int n_threads, int64_t window,
                m6a_prep_sites &P)
{
    if (n_norm < 0 || (n_norm > 0 && (!norm_kmers || !norm_mean || !norm_std))) return prep_fail(M6A_EINVAL, "bad normalisation arguments");
    const double t_all = now_ms();
    g_d2h = 0;
    DevMem m;
    m.advice = "run `dataprep` and then `inference` instead (the two-step path), or let --window_mb parse the file in windows";
    if (window < 0) window = window_from_env();
    double *ms = P.info.ms;
    int rc;
    if (n_paths == 1) {
        if ((rc = sites_impl(device_id, paths[0], rmin, rmax, min_seg, norm_kmers, norm_mean, norm_std, n_norm, host, n_threads, window, P, m, ms, nullptr)))
            return rc;
    } else {
        Pool pool(P.blob, P.tx_off);
        double bytes = 0;
        for (int f = 0; f < n_paths; f++) {
            double fm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if ((rc = sites_impl(device_id, paths[f], rmin, rmax, min_seg, norm_kmers, norm_mean, norm_std, n_norm, host, n_threads, window, P, m, fm, &pool)))
                return rc;
            for (int k = 0; k < 6; k++) ms[k] += fm[k];
            bytes += fm[6] * fm[0] * 1e6;
        }
        ms[6] = ms[0] > 0 ? bytes / (ms[0] * 1e6) : 0;
        if ((rc = pool_impl(pool, norm_kmers, n_norm, m, P, ms))) return rc;
    }
    ms[7] = now_ms() - t_all;
    P.info.d2h_bytes = g_d2h;
    P.info.peak_bytes = (int64_t)m.peak;
    return M6A_OK;
}

}  // namespace

// ---- grouped input (m6a_prep_group, include/m6a.h): sites as transcripts complete ---------------------------------------------------------
// The window loop stops between two windows.  After every window the host sees the names of the new segments (group_absorb: the
// grouped rule, the closed names) and the device says where the last contig stretch begins (group_closed); once the closed runs and
// rows reach the group size, the back half's stages run on them alone (group_batch), the closed part leaves the kept arrays
// (keep_tail) and the batch is cut on a flush boundary, the sites behind it carried in front of the next batch's (splice_sites).
namespace {
struct GroupSeg { int64_t first; int32_t len; uint32_t name; };    // a segment of the kept runs: its first run, the length and the number of its name
}

struct m6a_prep_group {
    int device = 0;
    std::string path, norm_kmers;
    std::vector<double> norm_mean, norm_std;
    int rmin = 0, rmax = 0, min_seg = 0, n_norm = 0, n_threads = 0;
    m6a_prep_host_half host{};
    bool has_host = false, stream = false, ended = false;
    int64_t group_bytes = 0, bs = 0, spb = 0;
    int failed = 0;                         // an error ends the group: every later call repeats it
    std::string failed_text;
    DevMem m;
    Streams S;
    Fd fd;
    std::unique_ptr<Windows> C;
    std::unique_ptr<Source> src;
    std::unique_ptr<WindowLoop> L;
    double fms[6] = {0, 0, 0, 0, 0, 0};
    std::string name_blob;                  // every contig name met so far, and whether another name has followed it
    std::vector<int64_t> name_off;
    Interner names{name_blob, name_off};
    std::vector<uint8_t> closed;
    int64_t cur = -1;
    std::vector<GroupSeg> segs;             // of the kept runs
    int64_t heads_seen = 0;                 // a stream: the saved contig bytes in front of this offset have been named
    int64_t closed_runs = 0, closed_rows = 0;
    m6a_prep_sites *carry = nullptr, *live = nullptr;
    int64_t written = 0;
    m6a_prep_group_counts n{};
    ~m6a_prep_group()
    {
        if (live) live->on_free = nullptr;
        delete carry;
        L.reset();
        src.reset();
        C.reset();
    }
};

namespace {

void group_batch_freed(void *owner, size_t bytes)
{
    m6a_prep_group *G = (m6a_prep_group *)owner;
    G->m.used -= std::min(bytes, G->m.used);
    G->live = nullptr;
}

// a handle the group made and no caller has seen
void group_drop(m6a_prep_group &G, m6a_prep_sites *&p)
{
    if (!p) return;
    G.m.used -= std::min(p->held, G.m.used);
    delete p;
    p = nullptr;
}

int group_open(m6a_prep_group &G, int64_t window)
{
    g_d2h = 0;
    G.m.advice = "run `dataprep` and then `inference` instead (the two-step path), or give a smaller --window_mb or M6A_PREP_GROUP_KB";
    int rc = open_device(G.device, G.m, nullptr);
    if (rc) return rc;
    const char *path = G.path.c_str();
    if (is_stdin(path)) { G.fd.fd = 0; G.fd.own = false; }
    else G.fd.fd = ::open(path, O_RDONLY);
    if (G.fd.fd < 0) return prep_fail(M6A_EIO, "cannot open %s", path);
    struct stat st;
    if (fstat(G.fd.fd, &st) != 0) return prep_fail(M6A_EIO, "cannot stat %s", path);
    G.stream = !S_ISREG(st.st_mode);
    const int64_t n = G.stream ? 0 : (int64_t)st.st_size;
    if (!G.stream && bgzf_is_gzip(G.fd.fd, n))
        return prep_fail(M6A_EINVAL, "%s: windows over compressed input are not implemented (--window_mb, M6A_PREP_WINDOW_KB); a BGZF file "
                         "must fit resident: run it without a window", path);
    if (window <= 0) window = window_from_env();
    if (window <= 0) window = M6A_PREP_STREAM_WINDOW_BYTES;
    const int64_t W = (window + kScanBytes - 1) / kScanBytes * kScanBytes;
    int64_t chunk = 0;
    if ((rc = G.S.open(W, chunk))) return rc;
    G.C.reset(new Windows(G.device, path, W, chunk, G.m, G.S));
    if (G.stream) G.src.reset(new StreamSource(*G.C, G.fd.fd));
    else G.src.reset(new FileSource(*G.C, G.fd.fd, n));
    G.L.reset(new WindowLoop(*G.C, *G.src, 1, false));
    G.L->ahead_fixed = 2.0;                                  // what is kept follows the group size, not the file's
    rc = G.L->start();
    G.n.d2h_bytes += g_d2h;
    return rc;
}

// the segments of the kept runs [NR0, NR): their names to the host, the grouped rule, the closed names
int group_absorb(m6a_prep_group &G, int64_t NR0)
{
    Kept &K = G.L->kept;
    DevMem &m = G.m;
    hipStream_t s = G.S.s[0];
    const int64_t n = K.NR - NR0;
    if (n <= 0) return M6A_OK;
    const RunDev *runs = (const RunDev *)K.runs.p + NR0;
    int rc;
    int64_t *sx, *dx, NSEG = 0, ND = 0;
    SegDev *seg;
    DeclDev *decl;
    if ((rc = m.alloc(sx, (size_t)n + 1, "segments")) || (rc = m.alloc(dx, (size_t)n + 1, "declined runs"))) return rc;
    if ((rc = launch(run_flags_kernel, n, s, runs, n, sx, dx))) return rc;
    if ((rc = scan_total(m, sx, n, s, NSEG)) || (rc = scan_total(m, dx, n, s, ND))) return rc;
    if ((rc = m.alloc(seg, (size_t)NSEG + 1, "segments")) || (rc = m.alloc(decl, (size_t)ND + 1, "declined runs"))) return rc;
    if ((rc = launch(run_lists_kernel, n, s, runs, n, sx, dx, seg, decl))) return rc;
    std::vector<SegDev> hseg((size_t)NSEG);
    if ((rc = d2h(hseg.data(), seg, (size_t)NSEG, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    m.release({sx, dx, seg, decl});
    int64_t total = 0;
    for (const SegDev &g : hseg) total += g.len;
    std::vector<char> bytes((size_t)total + 1);
    if (G.stream) {                                          // saved in run order: the new segments' names lie end to end
        if (G.heads_seen + total > (int64_t)K.heads.used) return prep_fail(M6A_EHIP, "the saved contig names of %s do not add up", G.path.c_str());
        if ((rc = d2h((uint8_t *)bytes.data(), K.heads.p + G.heads_seen, (size_t)total, s))) return rc;
        PCHK(hipStreamSynchronize(s));
        G.heads_seen += total;
    }
    std::string nm;
    int64_t at = 0;
    for (const SegDev &g : hseg) {
        if (G.stream) nm.assign(bytes.data() + at, (size_t)g.len);
        else {
            nm.resize((size_t)g.len);
            if ((rc = read_fully(G.fd.fd, &nm[0], g.len, g.contig, G.path.c_str()))) return rc;
        }
        at += g.len;
        const uint32_t id = G.names.id(nm);
        if (id == G.closed.size()) G.closed.push_back(0);
        if ((int64_t)id != G.cur) {
            if (G.cur >= 0) G.closed[(size_t)G.cur] = 1;
            if (G.closed[id])
                return prep_fail(M6A_EFORMAT, "%s: transcript %.*s appears again at byte %lld after other transcripts: the input is not grouped by "
                                 "transcript (run without --grouped)", G.path.c_str(), (int)std::min<size_t>(nm.size(), 256), nm.c_str(), (long long)g.contig);
            G.cur = id;
        }
        G.segs.push_back(GroupSeg{NR0 + g.first, g.len, id});
    }
    return M6A_OK;
}

// where the last contig stretch of the kept runs begins, and the rows in front of it
int group_closed(m6a_prep_group &G)
{
    Kept &K = G.L->kept;
    DevMem &m = G.m;
    hipStream_t s = G.S.s[0];
    const int64_t NSEG = (int64_t)G.segs.size();
    G.closed_runs = G.closed_rows = 0;
    if (NSEG < 2) return M6A_OK;
    std::vector<int64_t> first((size_t)NSEG);
    std::vector<uint32_t> rank((size_t)NSEG);
    for (int64_t g = 0; g < NSEG; g++) { first[(size_t)g] = G.segs[(size_t)g].first; rank[(size_t)g] = G.segs[(size_t)g].name; }
    int rc;
    int64_t *dfirst;
    uint32_t *drank;
    unsigned long long *out, h[2] = {0, 0};
    if ((rc = m.alloc(dfirst, (size_t)NSEG, "segments")) || (rc = m.alloc(drank, (size_t)NSEG, "segments")) || (rc = m.alloc(out, 2, "flags"))) return rc;
    if ((rc = h2d(dfirst, first.data(), (size_t)NSEG, s)) || (rc = h2d(drank, rank.data(), (size_t)NSEG, s))) return rc;
    PCHK(hipMemsetAsync(out, 0, 2 * sizeof(unsigned long long), s));
    if ((rc = launch(closed_prefix_kernel, NSEG, s, dfirst, drank, NSEG, out)) || (rc = fetch(h[0], out, s))) return rc;   // first and rank may go now
    const int64_t upto = (int64_t)h[0];
    if (upto < 0 || upto > K.NR) return prep_fail(M6A_EHIP, "the closed runs of %s do not add up", G.path.c_str());
    if ((rc = launch(rows_before_kernel, upto, s, (const int64_t *)K.cnt.p, upto, out + 1)) || (rc = fetch(h[1], out + 1, s))) return rc;
    m.release({dfirst, drank, out});
    if ((int64_t)h[1] > K.NROW) return prep_fail(M6A_EHIP, "the closed rows of %s do not add up", G.path.c_str());
    G.closed_runs = upto;
    G.closed_rows = (int64_t)h[1];
    return M6A_OK;
}

// what stays of a kept array when its first `from` bytes leave
int keep_tail(DevMem &m, hipStream_t s, DevVec &v, size_t from, const char *what)
{
    if (!v.p) return M6A_OK;
    if (from > v.used) return prep_fail(M6A_EHIP, "the kept %s do not add up", what);
    const size_t tail = v.used - from;
    uint8_t *q = nullptr;
    int rc = m.alloc(q, tail, what);
    if (rc) return rc;
    if ((rc = launch(keep_tail_kernel, (int64_t)((tail + 7) / 8), s, (const uint8_t *)v.p + from, (int64_t)tail, q))) return rc;
    PCHK(hipStreamSynchronize(s));
    m.release(v.p);
    v.p = q;
    v.cap = std::max<size_t>(16, tail);
    v.used = tail;
    return M6A_OK;
}

// sites [from, to) of A's followed by B's (either may be null) as a handle of their own: the carried sites go in front of a batch's
int splice_sites(m6a_prep_group &G, const m6a_prep_sites *A, const m6a_prep_sites *B, int64_t from, int64_t to, m6a_prep_sites *&out)
{
    DevMem &m = G.m;
    hipStream_t s = G.S.s[0];
    const int64_t NA = A ? A->info.n_sites : 0, RA = A ? A->info.n_reads : 0, NB = B ? B->info.n_sites : 0;
    if (from < 0 || to < from || to > NA + NB) return prep_fail(M6A_EHIP, "sites [%lld, %lld) of %lld", (long long)from, (long long)to, (long long)(NA + NB));
    auto reads_before = [&](int64_t i) { return i < NA ? A->off[(size_t)i] : RA + (B ? B->off[(size_t)(i - NA)] : 0); };
    const int64_t n = to - from, r0 = reads_before(from), R = reads_before(to) - r0;
    std::unique_ptr<m6a_prep_sites> P(new m6a_prep_sites);
    P->device = G.device;
    P->off.resize((size_t)n + 1); P->tx.resize((size_t)n); P->pos.resize((size_t)n); P->k7.resize((size_t)n * 7); P->ids.resize((size_t)R);
    Interner tx(P->blob, P->tx_off);
    std::vector<int64_t> map_a(A ? (size_t)A->info.n_tx : 0, -1), map_b(B ? (size_t)B->info.n_tx : 0, -1);
    for (int64_t j = 0; j < n; j++) {
        const int64_t i = from + j, k = i < NA ? i : i - NA;
        const m6a_prep_sites &Q = i < NA ? *A : *B;
        std::vector<int64_t> &map = i < NA ? map_a : map_b;
        const uint32_t t = Q.tx[(size_t)k];
        if (map[t] < 0) map[t] = tx.id(std::string(Q.blob.data() + Q.tx_off[t], (size_t)(Q.tx_off[t + 1] - Q.tx_off[t])));
        P->tx[(size_t)j] = (uint32_t)map[t];
        P->pos[(size_t)j] = Q.pos[(size_t)k];
        memcpy(P->k7.data() + j * 7, Q.k7.data() + k * 7, 7);
        P->off[(size_t)j] = reads_before(i) - r0;
    }
    P->off[(size_t)n] = R;
    P->tx_off.push_back((int64_t)P->blob.size());
    for (int64_t r = 0; r < R; r++) P->ids[(size_t)r] = r0 + r < RA ? A->ids[(size_t)(r0 + r)] : B->ids[(size_t)(r0 + r - RA)];
    P->rep.assign((size_t)R, 0);
    int rc;
    uint32_t *X, *stx;
    uint8_t *kmers, *sk7;
    int64_t *off, *spos;
    uint64_t *ids;
    float *rp, *sp;
    double *mr;
    if ((rc = m.alloc(X, (size_t)R * 9, "X")) || (rc = m.alloc(ids, (size_t)R + 1, "read ids")) || (rc = m.alloc(kmers, (size_t)n * 3 + 1, "site k-mers")) ||
        (rc = m.alloc(off, (size_t)n + 1, "the offsets")) || (rc = m.alloc(stx, (size_t)n + 1, "sites")) || (rc = m.alloc(spos, (size_t)n + 1, "sites")) ||
        (rc = m.alloc(sk7, (size_t)n * 7 + 1, "sites")) || (rc = m.alloc(rp, (size_t)R, "read probabilities")) ||
        (rc = m.alloc(sp, (size_t)n, "site probabilities")) || (rc = m.alloc(mr, (size_t)n, "mod ratios")))
        return rc;
    const m6a_prep_sites_info *IA = A ? &A->info : nullptr, *IB = B ? &B->info : nullptr;
    if ((rc = launch(splice_kernel<uint32_t>, R * 9, s, (const uint32_t *)(IA ? IA->X : nullptr), RA * 9, (const uint32_t *)(IB ? IB->X : nullptr), r0 * 9,
                     R * 9, X)) ||
        (rc = launch(splice_kernel<uint64_t>, R, s, (const uint64_t *)(A ? A->csv_ids : nullptr), RA, (const uint64_t *)(B ? B->csv_ids : nullptr), r0, R, ids)) ||
        (rc = launch(splice_kernel<uint8_t>, n * 3, s, IA ? IA->site_kmers : nullptr, NA * 3, IB ? IB->site_kmers : nullptr, from * 3, n * 3, kmers)) ||
        (rc = launch(splice_kernel<uint8_t>, n * 7, s, A ? A->csv_k7 : nullptr, NA * 7, B ? B->csv_k7 : nullptr, from * 7, n * 7, sk7)) ||
        (rc = launch(splice_kernel<int64_t>, n, s, A ? A->csv_pos : nullptr, NA, B ? B->csv_pos : nullptr, from, n, spos)) ||
        (rc = h2d(off, P->off.data(), (size_t)n + 1, s)) || (rc = h2d(stx, P->tx.data(), (size_t)n, s)))
        return rc;
    PCHK(hipStreamSynchronize(s));
    publish(*P, m, Result{n, R, (int64_t)tx.ids.size(), 1, (float *)X, kmers, off, rp, sp, mr, stx, spos, sk7, (const double *)ids, nullptr, nullptr, nullptr});
    out = P.release();
    return M6A_OK;
}

// The back half on the kept runs [0, NRc) alone, their removal, and the cut of the batch on a flush boundary.  *out stays null where no
// site can be delivered yet.
int group_batch(m6a_prep_group &G, int64_t NRc, bool final, m6a_prep_sites **out)
{
    Kept &K = G.L->kept;
    DevMem &m = G.m;
    hipStream_t s = G.S.s[0];
    int rc;
    m6a_prep_sites *raw = nullptr;
    struct Drop { m6a_prep_group &G; m6a_prep_sites *&p; ~Drop() { group_drop(G, p); } } drop_raw{G, raw};
    if (NRc > 0) {
        if (NRc > 0xffffffffll) return prep_fail(M6A_EINVAL, "more than 2^32 runs");
        const double t_all = now_ms();
        raw = new m6a_prep_sites;
        raw->device = G.device;
        const size_t mark = m.ptrs.size();
        int64_t rows = 0, heads_c = 0, decl_c = 0;
        {
            Back B(G.path.c_str(), G.rmin, G.rmax, G.has_host ? &G.host : nullptr, G.n_threads, *raw, m);
            B.fd.fd = G.fd.fd; B.fd.own = false;
            B.s = s;
            Front &F = B.F;
            int64_t *row_off;
            if ((rc = m.alloc(row_off, (size_t)NRc + 1, "rows"))) return rc;
            PCHK(hipMemcpyAsync(row_off, K.cnt.p, (size_t)NRc * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
            if ((rc = scan_total(m, row_off, NRc, s, rows))) return rc;
            for (const GroupSeg &g : G.segs)
                if (g.first < NRc) heads_c += g.len;
            if (rows > K.NROW || (G.stream && heads_c > (int64_t)K.heads.used)) return prep_fail(M6A_EHIP, "the closed rows of %s do not add up", G.path.c_str());
            F.NR = NRc; F.NROW = rows;
            F.runs = (RunDev *)K.runs.p; F.row_off = row_off;
            F.row_pos = (int64_t *)K.pos.p; F.row_kmer = K.kmer.p; F.row_feat = (double *)K.feat.p;
            F.stream = G.stream;
            F.heads = K.heads.p; F.n_heads = heads_c;
            F.declined = K.declined.p;
            B.NR = NRc; B.NROW = rows;
            B.t1 = now_ms();
            if ((rc = segments_to_host(B))) return rc;
            for (const DeclDev &d : B.hdecl) decl_c += d.end - d.start;
            if (G.stream && decl_c > (int64_t)K.declined.used) return prep_fail(M6A_EHIP, "the saved declined runs of %s do not add up", G.path.c_str());
            F.n_declined = decl_c;
            B.dev_ms += now_ms() - B.t1;
            B.t1 = now_ms();
            if ((rc = host_part(B, true))) return rc;
            B.host_ms += now_ms() - B.t1;
            B.t1 = now_ms();
            if ((rc = place_runs(B)) || (rc = sort_rows(B)) || (rc = cut_sites(B, std::max<int64_t>(G.min_seg, 20)))) return rc;
            if ((rc = finish_single(B, G.n_norm ? G.norm_kmers.data() : nullptr, G.n_norm ? G.norm_mean.data() : nullptr,
                                    G.n_norm ? G.norm_std.data() : nullptr, G.n_norm, raw->info.ms)))
                return rc;
            raw->info.ms[3] = B.dev_ms; raw->info.ms[4] = B.host_ms; raw->info.ms[7] = now_ms() - t_all;
        }
        PCHK(hipStreamSynchronize(s));
        m.release_since(mark, {});                           // the batch's own arrays are the handle's already
        // ---- the closed runs and rows leave the kept arrays
        if ((rc = keep_tail(m, s, K.runs, (size_t)NRc * sizeof(RunDev), "runs")) || (rc = keep_tail(m, s, K.cnt, (size_t)NRc * 8, "rows")) ||
            (rc = keep_tail(m, s, K.pos, (size_t)rows * 8, "rows")) || (rc = keep_tail(m, s, K.kmer, (size_t)rows * 7, "rows")) ||
            (rc = keep_tail(m, s, K.feat, (size_t)rows * 72, "rows")) || (rc = keep_tail(m, s, K.heads, (size_t)heads_c, "saved names")) ||
            (rc = keep_tail(m, s, K.declined, (size_t)decl_c, "saved runs")))
            return rc;
        K.NR -= NRc; K.NROW -= rows;
        size_t at = 0;
        for (const GroupSeg &g : G.segs)
            if (g.first >= NRc) { G.segs[at] = g; G.segs[at++].first -= NRc; }
        G.segs.resize(at);
        G.heads_seen -= heads_c;
        G.closed_runs = G.closed_rows = 0;
        G.n.total_runs += NRc; G.n.total_rows += rows;
    }
    // ---- the cut: every batch but the last ends on a flush boundary of the job, and what lies behind it heads the next
    const int64_t NC = G.carry ? G.carry->info.n_sites : 0, T = NC + (raw ? raw->info.n_sites : 0);
    int64_t cut = T;
    if (!final) {
        int64_t k = (G.written + T) / G.bs;
        while (k > 0 && k % G.spb == 0) --k;
        cut = std::max<int64_t>(k * G.bs - G.written, 0);
    }
    m6a_prep_sites *batch = nullptr, *rest = nullptr;
    if (cut == T && !NC) { batch = raw; raw = nullptr; }
    else if (cut == 0 && !NC) { rest = raw; raw = nullptr; }
    else {
        if (cut > 0 && (rc = splice_sites(G, G.carry, raw, 0, cut, batch))) return rc;
        if (cut < T && (rc = splice_sites(G, G.carry, raw, cut, T, rest))) { group_drop(G, batch); return rc; }
    }
    group_drop(G, G.carry);
    G.carry = rest;
    if (batch && batch->info.n_sites == 0) group_drop(G, batch);
    if (!batch) return M6A_OK;
    m6a_prep_sites_info &I = batch->info;
    I.n_windows = G.L->n_windows; I.window_bytes = G.L->w_max;
    I.peak_bytes = (int64_t)m.peak;
    I.d2h_bytes = G.n.d2h_bytes + g_d2h;
    batch->stream_bytes = G.n.stream_bytes; batch->n_streams = G.stream ? 1 : 0;
    batch->on_free = group_batch_freed;
    batch->owner = &G;
    G.live = batch;
    G.n.n_batches += 1; G.n.n_sites = I.n_sites; G.n.n_reads = I.n_reads; G.n.first_site = G.written;
    G.written += I.n_sites;
    *out = batch;
    return M6A_OK;
}

int group_next(m6a_prep_group &G, m6a_prep_sites **batch)
{
    g_d2h = 0;
    PCHK(hipSetDevice(G.device));
    Kept &K = G.L->kept;
    int rc = M6A_OK;
    for (;;) {
        const bool final = G.L->done;
        const int64_t bytes = G.closed_runs * (int64_t)(sizeof(RunDev) + 8) + G.closed_rows * (8 + 7 + 72);
        if (final || (G.closed_runs > 0 && bytes >= G.group_bytes)) {
            if ((rc = group_batch(G, final ? K.NR : G.closed_runs, final, batch))) break;
            if (final) G.ended = true;
            if (*batch || final) break;
            continue;
        }
        const int64_t NR0 = K.NR;
        if ((rc = G.L->step(G.fms))) break;
        G.n.n_windows = G.L->n_windows; G.n.window_bytes = G.L->w_max;
        G.n.max_kept_runs = std::max(G.n.max_kept_runs, K.NR); G.n.max_kept_rows = std::max(G.n.max_kept_rows, K.NROW);
        if ((rc = group_absorb(G, NR0))) break;
        if (G.L->done) {
            Front F;
            if ((rc = G.src->finish(G.L->b, F))) break;
            G.n.stream_bytes = F.stream ? F.n : 0;
        } else if ((rc = group_closed(G)))
            break;
    }
    G.n.d2h_bytes += g_d2h;
    G.n.peak_bytes = (int64_t)G.m.peak;
    return rc;
}

}  // namespace

extern "C" int m6a_prep_group_open(int device_id, const char *path, int readcount_min, int readcount_max, int min_segment_count,
                                   const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm,
                                   const m6a_prep_host_half *host, int n_threads, int64_t window_bytes, int64_t group_bytes, int64_t batch_size,
                                   int64_t save_per_batch, m6a_prep_group **out)
{
    if (!path || !out) return prep_fail(M6A_EINVAL, "null argument");
    *out = nullptr;
    if (n_norm < 0 || (n_norm > 0 && (!norm_kmers || !norm_mean || !norm_std))) return prep_fail(M6A_EINVAL, "bad normalisation arguments");
    if (batch_size < 1 || save_per_batch < 1) return prep_fail(M6A_EINVAL, "batch_size and save_per_batch must be 1 or more");
    return guarded([&]() -> int {
        std::unique_ptr<m6a_prep_group> G(new m6a_prep_group);
        G->device = device_id;
        G->path = path;
        G->rmin = readcount_min; G->rmax = readcount_max; G->min_seg = min_segment_count;
        G->n_norm = n_norm;
        if (n_norm) {
            G->norm_kmers.assign(norm_kmers, (size_t)n_norm * 5);
            G->norm_mean.assign(norm_mean, norm_mean + (size_t)n_norm * 3);
            G->norm_std.assign(norm_std, norm_std + (size_t)n_norm * 3);
        }
        if (host) { G->host = *host; G->has_host = true; }
        G->n_threads = n_threads;
        G->bs = batch_size; G->spb = save_per_batch;
        if (group_bytes <= 0) {
            const char *e = getenv("M6A_PREP_GROUP_KB");
            group_bytes = (e && atoll(e) > 0 ? atoll(e) : M6A_PREP_GROUP_KB_DEFAULT) << 10;
        }
        G->group_bytes = G->n.group_bytes = group_bytes;
        const int rc = group_open(*G, window_bytes);
        if (rc) return rc;
        *out = G.release();
        return M6A_OK;
    });
}

extern "C" int m6a_prep_group_next(m6a_prep_group *g, m6a_prep_sites **batch)
{
    if (!g || !batch) return prep_fail(M6A_EINVAL, "null argument");
    *batch = nullptr;
    if (g->failed) { g_prep_err = g->failed_text; return g->failed; }
    if (g->live) return prep_fail(M6A_EINVAL, "the batch before this one is still alive: free it before asking for the next");
    if (g->ended) return M6A_OK;
    const int rc = guarded([&] { return group_next(*g, batch); });
    if (rc) { g->failed = rc; g->failed_text = g_prep_err; }
    return rc;
}

extern "C" int m6a_prep_group_info(const m6a_prep_group *g, m6a_prep_group_counts *counts)
{
    if (!g || !counts) return prep_fail(M6A_EINVAL, "null argument");
    *counts = g->n;
    return M6A_OK;
}

extern "C" void m6a_prep_group_close(m6a_prep_group *g) { delete g; }

extern "C" int m6a_prep_eventalign(int device_id, const char *path, int n_neighbors, const char *index_path, m6a_prep **out)
{
    if (!path || !out) return prep_fail(M6A_EINVAL, "null argument");
    *out = nullptr;
    m6a_prep *p = new (std::nothrow) m6a_prep;
    if (!p) return prep_fail(M6A_ENOMEM, "out of host memory");
    const int rc = guarded([&] { return prep_impl(device_id, path, n_neighbors, index_path, *p); });
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

extern "C" int m6a_prep_sites_build(int device_id, const char *path, int readcount_min, int readcount_max, int min_segment_count,
                                    const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm,
                                    const m6a_prep_host_half *host, int n_threads, m6a_prep_sites **out)
{
    if (!path) return prep_fail(M6A_EINVAL, "null argument");
    return m6a_prep_sites_build_windows(device_id, &path, 1, readcount_min, readcount_max, min_segment_count, norm_kmers, norm_mean, norm_std,
                                        n_norm, host, n_threads, -1, out);
}

extern "C" int m6a_prep_sites_build_multi(int device_id, const char *const *paths, int n_paths, int readcount_min, int readcount_max,
                                          int min_segment_count, const char *norm_kmers, const double *norm_mean, const double *norm_std,
                                          int n_norm, const m6a_prep_host_half *host, int n_threads, m6a_prep_sites **out)
{
    return m6a_prep_sites_build_windows(device_id, paths, n_paths, readcount_min, readcount_max, min_segment_count, norm_kmers, norm_mean,
                                        norm_std, n_norm, host, n_threads, -1, out);
}

extern "C" int m6a_prep_sites_build_windows(int device_id, const char *const *paths, int n_paths, int readcount_min, int readcount_max,
                                            int min_segment_count, const char *norm_kmers, const double *norm_mean, const double *norm_std,
                                            int n_norm, const m6a_prep_host_half *host, int n_threads, int64_t window_bytes,
                                            m6a_prep_sites **out)
{
    return m6a_prep_sites_build_names(device_id, paths, n_paths, readcount_min, readcount_max, min_segment_count, norm_kmers, norm_mean,
                                      norm_std, n_norm, host, n_threads, window_bytes, 0, out);
}

extern "C" int m6a_prep_sites_build_names(int device_id, const char *const *paths, int n_paths, int readcount_min, int readcount_max,
                                          int min_segment_count, const char *norm_kmers, const double *norm_mean, const double *norm_std,
                                          int n_norm, const m6a_prep_host_half *host, int n_threads, int64_t window_bytes, int read_names,
                                          m6a_prep_sites **out)
{
    if (!paths || !out || n_paths < 1) return prep_fail(M6A_EINVAL, "null argument");
    for (int f = 0, n_stdin = 0; f < n_paths; f++) {
        if (!paths[f]) return prep_fail(M6A_EINVAL, "null argument");
        if (is_stdin(paths[f]) && ++n_stdin > 1)            // before anything is opened
            return prep_fail(M6A_EINVAL, "`-` is the standard input and can be read once: it is given twice");
    }
    *out = nullptr;
    m6a_prep_sites *p = new (std::nothrow) m6a_prep_sites;
    if (!p) return prep_fail(M6A_ENOMEM, "out of host memory");
    p->device = device_id;
    p->read_names = read_names != 0;
    const int rc = guarded([&] {
        return sites_multi(device_id, paths, n_paths, readcount_min, readcount_max, min_segment_count, norm_kmers, norm_mean, norm_std, n_norm, host,
                           n_threads, window_bytes, *p);
    });
    if (rc) { delete p; return rc; }
    *out = p;
    return M6A_OK;
}

extern "C" const m6a_prep_sites_info *m6a_prep_sites_get(const m6a_prep_sites *p) { return p ? &p->info : nullptr; }

extern "C" int m6a_prep_sites_read_names(const m6a_prep_sites *p, const uint8_t **names16, const int64_t **name_off, int *n_rep)
{
    if (!p || !names16 || !name_off || !n_rep) return prep_fail(M6A_EINVAL, "null argument");
    *names16 = p->read_names ? p->names16.data() : nullptr;
    *name_off = p->read_names ? p->name_off.data() : nullptr;
    *n_rep = p->read_names ? (int)p->name_off.size() - 1 : 0;
    return M6A_OK;
}

extern "C" double m6a_prep_sites_intern_ms(const m6a_prep_sites *p) { return p ? p->ms_intern : 0; }
extern "C" int64_t m6a_prep_sites_stream_bytes(const m6a_prep_sites *p) { return p ? p->stream_bytes : 0; }
extern "C" int64_t m6a_prep_sites_n_streams(const m6a_prep_sites *p) { return p ? p->n_streams : 0; }

extern "C" int m6a_prep_sites_fetch(m6a_prep_sites *p, float *read_prob, float *site_prob, double *mod_ratio)
{
    if (!p) return prep_fail(M6A_EINVAL, "null argument");
    const int64_t R = p->info.n_reads, S = p->info.n_sites;
    if ((R && !read_prob) || (S && (!site_prob || !mod_ratio))) return prep_fail(M6A_EINVAL, "null argument");
    const double t = now_ms();
    PCHK(hipSetDevice(p->device));
    if (R) PCHK(hipMemcpy(read_prob, p->info.read_prob, (size_t)R * sizeof(float), hipMemcpyDeviceToHost));
    if (S) PCHK(hipMemcpy(site_prob, p->info.site_prob, (size_t)S * sizeof(float), hipMemcpyDeviceToHost));
    if (S) PCHK(hipMemcpy(mod_ratio, p->info.mod_ratio, (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    p->info.d2h_bytes += R * (int64_t)sizeof(float) + S * (int64_t)(sizeof(float) + sizeof(double));
    p->info.ms[5] += now_ms() - t;
    return M6A_OK;
}

extern "C" int m6a_prep_sites_inputs(m6a_prep_sites *p, float *X, uint8_t *site_kmers, int64_t *off)
{
    if (!p || !X || !site_kmers || !off) return prep_fail(M6A_EINVAL, "null argument");
    const int64_t R = p->info.n_reads, S = p->info.n_sites;
    PCHK(hipSetDevice(p->device));
    if (R) PCHK(hipMemcpy(X, p->info.X, (size_t)R * 9 * sizeof(float), hipMemcpyDeviceToHost));
    if (S) PCHK(hipMemcpy(site_kmers, p->info.site_kmers, (size_t)S * 3, hipMemcpyDeviceToHost));
    PCHK(hipMemcpy(off, p->info.off, (size_t)(S + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    p->info.d2h_bytes += R * 36 + S * 3 + (S + 1) * 8;
    return M6A_OK;
}

extern "C" void m6a_prep_sites_free(m6a_prep_sites *p) { delete p; }

#define M6A_BGZF_DEVICE_PART
#include "m6a_bgzf.h"
#include "m6a_csv.h"
#include "m6a_npy_write.h"
#include "m6a_dataprep.h"
#define M6A_DEFLATE_DEVICE_PART
#include "m6a_deflate.h"
#define M6A_JSON_DEVICE_PART
#include "m6a_json.h"
#define M6A_NORM_DEVICE_PART
#include "m6a_norm.h"
