// m6a_dataprep.h -- eventalign.index, data.json, data.info and data.log written from the device (include/m6a.h: m6a_repr_format,
// m6a_prep_dataprep_write).  Part of m6a_prep.hip's translation unit, behind m6a_csv.h (it uses that file's csv_emit and pwrite
// helpers, m6a_prep_kit.h's DevMem, scans, Rounds and run_rounds, and m6a_prep.hip's RowSrc and RunDev); not a file to compile on its own.
//
// The bytes are the host writer's (m6a_io.cpp: emit_transcript, dataprep_impl); the numbers are m6a_repr.h's.
//   record     {"<tx>":{"<pos>":{"<7-mer>":[[f,f,f,f,f,f,f,f,f,<read>.0],[...]]}}}\n  per kept site; as rows for csv_emit a site is its
//              reads: read 0 carries the head up to `":[`, every later read a leading comma, the last read the tail `]}}}\n`
//   index row  <tx>,<read>,<start>,<end>\n per run, in file order
// Rows have different lengths, so either file takes the CSV writer's three steps:
//   lengths    json_len_kernel, a wave per kept site, lanes over its reads: the length of the record, and the count of values the
//              number core DECLINES (m6a_repr.h); index_len_kernel, a lane per run
//   offsets    exclusive 64-bit scans (scan_excl): every record's [start, end) in data.json -- data.info's columns -- and both file
//              sizes, before a file is opened
//   write      json_write_kernel, a wave per site, and index_write_kernel, a wave per 64 runs: csv_emit stages up to 64 rows in a
//              tile of LDS and stores aligned dwords
// dataprep_emit is the way out of sites_impl for `dataprep --writer device`: where the inference path would build X, the sorted row
// list (L, src, off) is printed instead, in rounds of whole sites bounded by M6A_JSON_ROUND_KB of text, double-buffered in pinned
// memory as csv_write_impl's are; eventalign.index follows through the same two buffers in rounds of whole blocks of rows (the
// offsets stay on the device: one offset per block of rows comes back).  data.info and data.log are printed on the host from
// 28 bytes per kept site and one byte per transcript.
#pragma once

#include "m6a_repr.h"

namespace {

constexpr int64_t kJsonRoundKB = 32768;    // default M6A_JSON_ROUND_KB

// the reads of one site as rows of text
struct JsonRows {
    const JsonDev &d;
    int64_t l0, n, pos, name_len;
    const uint8_t *name, *k7;

    __device__ JsonRows(const JsonDev &d_, int64_t i) : d(d_)
    {
        l0 = d.src[i];
        n = d.off[i + 1] - d.off[i];
        pos = d.site_pos[i];
        const int64_t t0 = d.tx_off[d.site_tx[i]];
        name = d.tx_blob + t0;
        name_len = d.tx_off[d.site_tx[i] + 1] - t0;
        k7 = d.site_k7 + i * 7;
    }
    __device__ int64_t len(int64_t j, unsigned &declined) const
    {
        const uint32_t row = d.L[l0 + j];
        const double *f = d.rs.feat(row);
        int64_t k = j == 0 ? 2 + name_len + 4 + m6a_repr::i64<false>(pos, nullptr) + 4 + 7 + 3 : 1;
        k += 1 + 9 + 1;                                     // [ nine commas ]
        for (int c = 0; c < 9; c++) {
            const int q = m6a_repr::feature<false>(f[c], d.round3, nullptr);
            if (q < 0) declined++; else k += q;
        }
        const int q = m6a_repr::read_id<false>(d.runs[d.row_run[row]].read, nullptr);
        if (q < 0) declined++; else k += q;
        return k + (j == n - 1 ? 5 : 0);
    }
    __device__ int64_t len(int64_t j) const { unsigned x = 0; return len(j, x); }
    __device__ void put(int64_t j, char *o) const
    {
        const uint32_t row = d.L[l0 + j];
        const double *f = d.rs.feat(row);
        if (j == 0) {
            *o++ = '{'; *o++ = '"';
            for (int64_t c = 0; c < name_len; c++) o[c] = (char)name[c];
            o += name_len;
            *o++ = '"'; *o++ = ':'; *o++ = '{'; *o++ = '"';
            o += m6a_repr::i64<true>(pos, o);
            *o++ = '"'; *o++ = ':'; *o++ = '{'; *o++ = '"';
            for (int c = 0; c < 7; c++) *o++ = (char)k7[c];
            *o++ = '"'; *o++ = ':'; *o++ = '[';
        } else {
            *o++ = ',';
        }
        *o++ = '[';
        for (int c = 0; c < 9; c++) {
            const int q = m6a_repr::feature<true>(f[c], d.round3, o);
            if (q > 0) o += q;                              // (a declined value is never written out: the call ends before any text)
            *o++ = ',';
        }
        const int q = m6a_repr::read_id<true>(d.runs[d.row_run[row]].read, o);
        if (q > 0) o += q;
        *o++ = ']';
        if (j == n - 1) { *o++ = ']'; *o++ = '}'; *o++ = '}'; *o++ = '}'; *o++ = '\n'; }
    }
};

struct IndexDev {
    const RunDev *runs;
    const uint32_t *run_tx;
    const uint8_t *tx_blob;
    const int64_t *tx_off;
};

// the rows of eventalign.index from run `first` on
struct IndexRows {
    const IndexDev &d;
    int64_t first;

    __device__ int64_t len(int64_t j) const
    {
        const RunDev &R = d.runs[first + j];
        const uint32_t t = d.run_tx[first + j];
        return d.tx_off[t + 1] - d.tx_off[t] + 4 + m6a_repr::i64<false>(R.read, nullptr) + m6a_repr::i64<false>(R.start, nullptr) +
               m6a_repr::i64<false>(R.end, nullptr);
    }
    __device__ void put(int64_t j, char *o) const
    {
        const RunDev &R = d.runs[first + j];
        const uint32_t t = d.run_tx[first + j];
        const int64_t t0 = d.tx_off[t], nl = d.tx_off[t + 1] - t0;
        for (int64_t c = 0; c < nl; c++) o[c] = (char)d.tx_blob[t0 + c];
        o += nl;
        *o++ = ',';
        o += m6a_repr::i64<true>(R.read, o);
        *o++ = ',';
        o += m6a_repr::i64<true>(R.start, o);
        *o++ = ',';
        o += m6a_repr::i64<true>(R.end, o);
        *o = '\n';
    }
};

// m6a_repr_format: values [first, ...) back to back; a declined value is a row of no bytes
struct ReprRows {
    const double *v;
    int64_t first;
    int round3;
    __device__ int64_t len(int64_t j) const
    {
        const int q = m6a_repr::feature<false>(v[first + j], round3, nullptr);
        return q < 0 ? 0 : q;
    }
    __device__ void put(int64_t j, char *o) const { (void)m6a_repr::feature<true>(v[first + j], round3, o); }
};

__global__ __launch_bounds__(kCsvWave) void json_len_kernel(JsonDev d, int64_t S, int64_t *__restrict__ len, unsigned long long *__restrict__ declined)
{
    const int64_t i = blockIdx.x;
    if (i >= S) return;
    const int lane = (int)threadIdx.x;
    const JsonRows rows(d, i);
    int64_t sum = 0;
    unsigned decl = 0;
    for (int64_t j = lane; j < rows.n; j += kCsvWave) sum += rows.len(j, decl);
    for (int o = kCsvWave / 2; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        decl += __shfl_xor(decl, o);
    }
    if (lane == 0) {
        len[i] = sum;
        if (decl) atomicAdd(declined, (unsigned long long)decl);
    }
}

// joff: the scanned lengths of all sites; the text of sites [a, b) lands in `out` from byte 0 on
__global__ __launch_bounds__(kCsvWave) void json_write_kernel(JsonDev d, int64_t a, int64_t b, const int64_t *__restrict__ joff, char *__restrict__ out)
{
    __shared__ uint32_t lds[(kCsvTile + 8) / 4];
    const int64_t i = a + blockIdx.x;
    if (i >= b) return;
    const JsonRows rows(d, i);
    csv_emit(out, joff[i] - joff[a], rows.n, rows, lds);
}

// one flag per transcript: it has a candidate row among the used runs (`logged` in emit_transcript)
__global__ void tx_logged_kernel(const uint32_t *__restrict__ L, int64_t n, const uint32_t *__restrict__ row_run, const uint32_t *__restrict__ run_tx,
                                 uint8_t *__restrict__ logged)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i < n) logged[run_tx[row_run[L[i]]]] = 1;
}

__global__ void index_len_kernel(IndexDev d, int64_t NR, int64_t *__restrict__ len)
{
    const int64_t r = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (r < NR) len[r] = IndexRows{d, 0}.len(r);
}

// every q-th offset, and the last: out[c] = xoff[min(c q, NR)]
__global__ void index_cut_kernel(const int64_t *__restrict__ xoff, int64_t NR, int64_t q, int64_t nc, int64_t *__restrict__ out)
{
    const int64_t c = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (c < nc) out[c] = xoff[c * q < NR ? c * q : NR];
}

__global__ __launch_bounds__(kCsvWave) void index_write_kernel(IndexDev d, int64_t a, int64_t b, const int64_t *__restrict__ xoff, char *__restrict__ out)
{
    __shared__ uint32_t lds[(kCsvTile + 8) / 4];
    const int64_t r = a + (int64_t)blockIdx.x * kCsvWave;
    if (r >= b) return;
    csv_emit(out, xoff[r] - xoff[a], b - r < kCsvWave ? b - r : (int64_t)kCsvWave, IndexRows{d, r}, lds);
}

__global__ void repr_len_kernel(const double *__restrict__ v, int64_t n, int round3, int64_t *__restrict__ len, unsigned long long *__restrict__ declined)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    const int q = m6a_repr::feature<false>(v[i], round3, nullptr);
    len[i] = q < 0 ? 0 : q;
    if (q < 0) atomicAdd(declined, 1ull);
}

__global__ __launch_bounds__(kCsvWave) void repr_write_kernel(const double *__restrict__ v, int64_t n, int round3, const int64_t *__restrict__ off,
                                                              char *__restrict__ out)
{
    __shared__ uint32_t lds[(kCsvTile + 8) / 4];
    const int64_t i = (int64_t)blockIdx.x * kCsvWave;
    if (i >= n) return;
    csv_emit(out, off[i], n - i < kCsvWave ? n - i : (int64_t)kCsvWave, ReprRows{v, i, round3}, lds);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

// files this call created: removed again unless it succeeds
struct DataprepFiles {
    std::string path[4];                   // eventalign.index, data.json, data.info, data.log
    int fd[4] = {-1, -1, -1, -1};
    bool keep = false;
    int open_all(const char *out_dir)
    {
        const char *names[4] = {"eventalign.index", "data.json", "data.info", "data.log"};
        for (int i = 0; i < 4; i++) {
            path[i] = std::string(out_dir) + "/" + names[i];
            fd[i] = ::open(path[i].c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            if (fd[i] < 0) return prep_fail(M6A_EIO, "cannot write into %s", out_dir);
        }
        return M6A_OK;
    }
    int close_all(const char *out_dir)
    {
        int bad = 0;
        for (int i = 0; i < 4; i++)
            if (fd[i] >= 0) { bad |= ::close(fd[i]); fd[i] = -1; }
        return bad ? prep_fail(M6A_EIO, "cannot close outputs in %s", out_dir) : M6A_OK;
    }
    ~DataprepFiles()
    {
        for (int i = 0; i < 4; i++) {
            if (fd[i] >= 0) (void)::close(fd[i]);
            if (!keep && !path[i].empty()) (void)::unlink(path[i].c_str());
        }
    }
};

// rounds [cut[k], cut[k + 1]) of items whose text starts at byte at[k] of the items' text
struct TextRounds {
    std::vector<int64_t> cut{0}, at{0};
    int64_t cap = 0;
    int64_t n() const { return (int64_t)cut.size() - 1; }
    void add(int64_t item_end, int64_t byte_end)
    {
        cap = std::max(cap, byte_end - at.back());
        cut.push_back(item_end);
        at.push_back(byte_end);
    }
};

// round k + 1 is formatted and copied while round k is written at file offset base + at[k]; events: start, formatted, copied
template <class Launch>
int text_rounds_write(const TextRounds &T, Rounds &rd, char *const dbuf[2], Launch launch, int fd, int64_t base, int nw, const char *path,
                      m6a_dataprep_stats &st)
{
    auto queue = [&](int64_t k) -> int {
        const int i = (int)(k & 1);
        PCHK(hipEventRecord(rd.e[i][0], rd.s[i]));
        const int rc = launch(T.cut[(size_t)k], T.cut[(size_t)k + 1], dbuf[i], rd.s[i]);
        if (rc) return rc;
        PCHK(hipEventRecord(rd.e[i][1], rd.s[i]));
        const int64_t n = T.at[(size_t)k + 1] - T.at[(size_t)k];
        if (n) PCHK(hipMemcpyAsync(rd.pin[i], dbuf[i], (size_t)n, hipMemcpyDeviceToHost, rd.s[i]));
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
        const double t0 = now_ms();
        if (!csv_pwrite_threads(fd, rd.pin[i], T.at[(size_t)k + 1] - T.at[(size_t)k], base + T.at[(size_t)k], nw)) return prep_fail(M6A_EIO, "cannot write %s", path);
        st.ms_write += now_ms() - t0;
        return M6A_OK;
    };
    const int rc = run_rounds(T.n(), queue, finish);
    if (!rc) st.n_rounds += T.n();
    return rc;
}

const char kIndexHeader[] = "transcript_id,read_index,pos_start,pos_end\n";
const char kInfoHeader[] = "transcript_id,transcript_position,start,end,n_reads\n";

int dataprep_emit(DevMem &m, hipStream_t s0, const DataprepJob &job, const DataprepSrc &src)
{
    m6a_dataprep_stats &st = *job.st;
    const int64_t NS = src.NS, NR = src.NR, NT = src.NT;
    const int nw = job.n_threads > 0 ? job.n_threads : m6a_usable_cpus();
    if (NS > 0x7fffffffll) return prep_fail(M6A_EINVAL, "more than 2^31 sites");
    st.n_sites = NS;
    st.n_runs = NR;
    Rounds rd;
    int rc = rd.open(3);
    if (rc) return rc;
    PCHK(hipStreamSynchronize(s0));                         // the back half's arrays are complete
    hipStream_t s = rd.s[0];
    double t0 = now_ms();

    // ---- the small uploads, lengths and offsets of the whole job
    uint8_t *blob, *logged;
    int64_t *tx_off, *joff, *xoff, *xcut;
    unsigned long long *dd, hd = 0;
    const size_t nblob = src.blob->size();
    if ((rc = m.alloc(blob, nblob + 1, "transcript names")) || (rc = m.alloc(tx_off, (size_t)NT + 1, "transcript names")) ||
        (rc = m.alloc(logged, (size_t)NT + 1, "transcripts")) || (rc = m.alloc(joff, (size_t)NS + 1, "data.json offsets")) ||
        (rc = m.alloc(xoff, (size_t)NR + 1, "index offsets")) || (rc = m.alloc(dd, 1, "flags")))
        return rc;
    if ((rc = h2d(blob, (const uint8_t *)src.blob->data(), nblob, s)) || (rc = h2d(tx_off, src.tx_off->data(), (size_t)NT + 1, s))) return rc;
    PCHK(hipMemsetAsync(logged, 0, (size_t)NT + 1, s));
    PCHK(hipMemsetAsync(dd, 0, sizeof *dd, s));
    PCHK(hipMemsetAsync(joff + NS, 0, sizeof(int64_t), s));
    PCHK(hipMemsetAsync(xoff + NR, 0, sizeof(int64_t), s));
    JsonDev jd = src.json;
    jd.tx_blob = blob;
    jd.tx_off = tx_off;
    jd.round3 = job.compress ? 1 : 0;
    const IndexDev xd{jd.runs, src.run_tx, blob, tx_off};
    if (src.NL) {
        tx_logged_kernel<<<grid(src.NL), kBlk, 0, s>>>(jd.L, src.NL, jd.row_run, src.run_tx, logged);
        PCHK(hipGetLastError());
    }
    if (NS) {
        json_len_kernel<<<(unsigned)NS, kCsvWave, 0, s>>>(jd, NS, joff, dd);
        PCHK(hipGetLastError());
    }
    if (NR) {
        index_len_kernel<<<grid(NR), kBlk, 0, s>>>(xd, NR, xoff);
        PCHK(hipGetLastError());
    }
    if ((rc = scan_excl(m, joff, NS + 1, s)) || (rc = scan_excl(m, xoff, NR + 1, s))) return rc;
    const int64_t round_bytes = round_kb("M6A_JSON_ROUND_KB", kJsonRoundKB) << 10;
    // index rows come back as one offset per block of q rows (q rows are about a sixteenth of a round)
    const int64_t q = std::max<int64_t>(kCsvWave, round_bytes / 1024), nc = (NR + q - 1) / q + 1;
    if ((rc = m.alloc(xcut, (size_t)nc, "index offsets"))) return rc;
    index_cut_kernel<<<grid(nc), kBlk, 0, s>>>(xoff, NR, q, nc, xcut);
    PCHK(hipGetLastError());
    std::vector<int64_t> hj((size_t)NS + 1), hcut((size_t)nc), hpos((size_t)NS), hoff((size_t)NS + 1);
    std::vector<uint32_t> htx((size_t)NS);
    std::vector<uint8_t> hlog((size_t)NT);
    if ((rc = d2h(hj.data(), joff, (size_t)NS + 1, s)) || (rc = d2h(hcut.data(), xcut, (size_t)nc, s)) || (rc = d2h(&hd, dd, 1, s)) ||
        (rc = d2h(hpos.data(), jd.site_pos, (size_t)NS, s)) || (rc = d2h(htx.data(), jd.site_tx, (size_t)NS, s)) ||
        (rc = d2h(hoff.data(), jd.off, (size_t)NS + 1, s)) || (rc = d2h(hlog.data(), logged, (size_t)NT, s)))
        return rc;
    PCHK(hipStreamSynchronize(s));
    st.ms_format += now_ms() - t0;
    st.n_declined = (int64_t)hd;
    st.json_bytes = hj[(size_t)NS];
    st.index_bytes = hcut[(size_t)nc - 1] + (int64_t)sizeof(kIndexHeader) - 1;
    if (hd)
        return prep_fail(M6A_EDECLINED, "%lld values are outside what the device prints (a feature that is not a finite value with 1e-4 <= v < 1e16, "
                         "a read index outside [0, 2^53))", (long long)hd);

    // ---- rounds of whole sites, and of whole blocks of index rows
    TextRounds J, X;
    m6a_rounds::cut_rounds(NS, round_bytes, [&](int64_t a, int64_t b) { return hj[(size_t)b] - hj[(size_t)a]; },
                           [&](int64_t, int64_t b) { J.add(b, hj[(size_t)b]); });
    for (int64_t c = 0; c + 1 < nc;) {
        int64_t e = c + 1;
        while (e + 1 < nc && hcut[(size_t)e + 1] - hcut[(size_t)c] <= round_bytes) ++e;
        X.add(std::min(e * q, NR), hcut[(size_t)e]);
        c = e;
    }
    const int64_t cap = std::max<int64_t>(std::max(J.cap, X.cap), 16);
    char *dbuf[2] = {nullptr, nullptr};
    for (int i = 0; i < (J.n() > 1 || X.n() > 1 ? 2 : 1); i++) {
        if ((rc = m.alloc(dbuf[i], (size_t)cap, "text")) || (rc = rd.pinned(i, cap))) return rc;
    }

    // ---- the files
    DataprepFiles F;
    if ((rc = F.open_all(job.out_dir))) return rc;
    auto json_launch = [&](int64_t a, int64_t b, char *out, hipStream_t rs) -> int {
        if (b <= a) return M6A_OK;
        json_write_kernel<<<(unsigned)(b - a), kCsvWave, 0, rs>>>(jd, a, b, joff, out);
        PCHK(hipGetLastError());
        return M6A_OK;
    };
    auto index_launch = [&](int64_t a, int64_t b, char *out, hipStream_t rs) -> int {
        if (b <= a) return M6A_OK;
        index_write_kernel<<<(unsigned)((b - a + kCsvWave - 1) / kCsvWave), kCsvWave, 0, rs>>>(xd, a, b, xoff, out);
        PCHK(hipGetLastError());
        return M6A_OK;
    };
    if ((rc = text_rounds_write(J, rd, dbuf, json_launch, F.fd[1], 0, nw, F.path[1].c_str(), st))) return rc;
    if (!csv_pwrite_all(F.fd[0], kIndexHeader, (int64_t)sizeof(kIndexHeader) - 1, 0)) return prep_fail(M6A_EIO, "cannot write %s", F.path[0].c_str());
    if ((rc = text_rounds_write(X, rd, dbuf, index_launch, F.fd[0], (int64_t)sizeof(kIndexHeader) - 1, nw, F.path[0].c_str(), st))) return rc;

    // ---- data.info and data.log, on the host
    t0 = now_ms();
    const std::string &names = *src.blob;
    const std::vector<int64_t> &to = *src.tx_off;
    std::string text = kInfoHeader;
    char num[96];
    for (int64_t i = 0; i < NS; i++) {
        const uint32_t t = htx[(size_t)i];
        text.append(names, (size_t)to[t], (size_t)(to[t + 1] - to[t]));
        const int k = snprintf(num, sizeof num, ",%lld,%lld,%lld,%lld\n", (long long)hpos[(size_t)i], (long long)hj[(size_t)i], (long long)hj[(size_t)i + 1],
                               (long long)(hoff[(size_t)i + 1] - hoff[(size_t)i]));
        text.append(num, (size_t)k);
        if (text.size() >= ((size_t)4 << 20) || i == NS - 1) {
            if ((rc = write_fully(F.fd[2], text.data(), text.size(), F.path[2].c_str()))) return rc;
            text.clear();
        }
    }
    if (!text.empty() && (rc = write_fully(F.fd[2], text.data(), text.size(), F.path[2].c_str()))) return rc;
    text.clear();
    for (int64_t t = 0; t < NT; t++) {
        if (!hlog[(size_t)t]) continue;
        text.append(names, (size_t)to[(size_t)t], (size_t)(to[(size_t)t + 1] - to[(size_t)t]));
        text += ": Data preparation ... Done.\n";
    }
    if ((rc = write_fully(F.fd[3], text.data(), text.size(), F.path[3].c_str()))) return rc;
    if ((rc = F.close_all(job.out_dir))) return rc;
    st.ms_write += now_ms() - t0;
    F.keep = true;
    return M6A_OK;
}

int repr_format_impl(int device_id, const double *v, int64_t n, int round3, char *text, int64_t cap, int64_t *off, int64_t *n_declined)
{
    if (n < 0 || (n && !v) || !off || !n_declined) return prep_fail(M6A_EINVAL, "null argument");
    if (n > 0x7fffffffll * kCsvWave) return prep_fail(M6A_EINVAL, "more than 2^37 values");
    DevMem m;
    int rc = open_device(device_id, m, "format fewer values per call");
    if (rc) return rc;
    Streams st;
    PCHK(hipStreamCreateWithFlags(&st.s[0], hipStreamNonBlocking));
    hipStream_t s = st.s[0];
    double *dv;
    int64_t *doff;
    unsigned long long *dd, hd = 0;
    if ((rc = m.alloc(dv, (size_t)n, "values")) || (rc = m.alloc(doff, (size_t)n + 1, "offsets")) || (rc = m.alloc(dd, 1, "flags"))) return rc;
    if ((rc = h2d(dv, v, (size_t)n, s))) return rc;
    PCHK(hipMemsetAsync(dd, 0, sizeof *dd, s));
    PCHK(hipMemsetAsync(doff + n, 0, sizeof(int64_t), s));
    if (n) {
        repr_len_kernel<<<grid(n), kBlk, 0, s>>>(dv, n, round3 ? 1 : 0, doff, dd);
        PCHK(hipGetLastError());
    }
    if ((rc = scan_excl(m, doff, n + 1, s))) return rc;
    if ((rc = d2h(off, doff, (size_t)n + 1, s)) || (rc = d2h(&hd, dd, 1, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    *n_declined = (int64_t)hd;
    if (!text) return M6A_OK;                               // the sizing call
    if (cap < off[n]) return prep_fail(M6A_EINVAL, "the text takes %lld bytes, the buffer holds %lld", (long long)off[n], (long long)cap);
    char *out;
    if ((rc = m.alloc(out, (size_t)off[n] + 4, "text"))) return rc;
    if (n) {
        repr_write_kernel<<<(unsigned)((n + kCsvWave - 1) / kCsvWave), kCsvWave, 0, s>>>(dv, n, round3 ? 1 : 0, doff, out);
        PCHK(hipGetLastError());
    }
    if ((rc = d2h(text, out, (size_t)off[n], s))) return rc;
    PCHK(hipStreamSynchronize(s));
    return M6A_OK;
}

}  // namespace

extern "C" int m6a_repr_format(int device_id, const double *v, int64_t n, int round3, char *text, int64_t cap, int64_t *off, int64_t *n_declined)
{
    return guarded([&] { return repr_format_impl(device_id, v, n, round3, text, cap, off, n_declined); });
}

extern "C" int m6a_prep_dataprep_write(int device_id, const char *path, const char *out_dir, int readcount_min, int readcount_max,
                                       int min_segment_count, int compress, const m6a_prep_host_half *host, int n_threads,
                                       m6a_dataprep_stats *stats)
{
    m6a_dataprep_stats st{};
    int rc;
    if (!path || !out_dir) rc = prep_fail(M6A_EINVAL, "null argument");
    else
        rc = guarded([&] {
            g_d2h = 0;
            DevMem m;                                       // its advice is the budget error's `use --device cpu`
            m6a_prep_sites P;
            P.device = device_id;
            const DataprepJob job{out_dir, compress, n_threads, &st};
            double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const int rc2 = sites_impl(device_id, path, readcount_min, readcount_max, min_segment_count, nullptr, nullptr, nullptr, 0, host,
                                       n_threads, window_from_env(), P, m, ms, nullptr, &job);
            st.d2h_bytes = g_d2h;
            st.peak_bytes = (int64_t)m.peak;
            return rc2;
        });
    if (stats) *stats = st;
    return rc;
}
