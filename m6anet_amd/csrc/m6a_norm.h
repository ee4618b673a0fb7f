// m6a_norm.h -- the summation core of `compute_norm_factors` (include/m6a.h states the operation at m6a_norm_factors_build): the
// column sum in the order np.sum adds a Fortran-contiguous column, and the finish, as plain C++ marked for host and device.
// m6a_io.cpp compiles it for the CPU (m6a_io_norm_factors), tests/norm_core_main.cpp holds it to tests/norm_statement.py as a program
// of its own under ASan and UBSan, and m6a_prep.hip compiles the same text for gfx950 (norm_sums_kernel).
//   colsum   the column is cut into pieces of 8 192 elements (NumPy's reduce buffer); the first piece's sum, then every later
//            piece's sum added to it in order.  A piece is summed pairwise:
//              n < 8          sequentially from 0.0
//              8 <= n <= 128  eight accumulators r[j] = a[j], r[j] += a[i + j] for i = 8, 16, ... below n - n % 8,
//                             ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the last n % 8 elements one by one
//              n > 128        n2 = n / 2 less n2 % 8; the sum of the first n2 plus the sum of the rest
//            The recursion is walked with a stack of its own (no recursive call on the device); what sums a leaf (n <= 128) is the
//            caller's: leaf() below on the host, a lane per accumulator in the kernel.
//   finish   mean = S / N, std = sqrt(S2 / N - mean * mean): one IEEE operation each (build with -ffp-contract=off), NaN for a
//            negative argument.
#ifndef M6A_NORM_H
#define M6A_NORM_H
#include <math.h>
#include <stdint.h>

#ifndef M6A_HD
#if defined(__HIPCC__)
#define M6A_HD __host__ __device__
#else
#define M6A_HD
#endif
#endif

namespace m6a_norm {

constexpr int64_t kPiece = 8192, kLeaf = 128;
constexpr int kDepth = 24;                 // of the walk's stack: pieces of 8 192 need 8

// elements [lo, lo + n) of get, n <= kLeaf
template <class Get>
M6A_HD inline double leaf(Get &&get, int64_t lo, int64_t n)
{
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; i++) res += get(lo + i);
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; j++) r[j] = get(lo + j);
    int64_t i;
    for (i = 8; i < n - n % 8; i += 8)
        for (int j = 0; j < 8; j++) r[j] += get(lo + i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += get(lo + i);
    return res;
}

// the pairwise sum of [lo, lo + n): leaf_sum(lo, n) is asked for every leaf, left to right
template <class LeafSum>
M6A_HD inline double pairwise(LeafSum &&leaf_sum, int64_t lo, int64_t n)
{
    if (n <= kLeaf) return leaf_sum(lo, n);
    struct Frame { int64_t lo, n; double left; int state; } st[kDepth];
    int sp = 1;
    double ret = 0.0;
    st[0] = Frame{lo, n, 0.0, 0};
    while (sp > 0) {
        Frame &f = st[sp - 1];
        if (f.n <= kLeaf) {
            ret = leaf_sum(f.lo, f.n);
            --sp;
            continue;
        }
        int64_t n2 = f.n / 2;
        n2 -= n2 % 8;
        if (f.state == 0) {
            f.state = 1;
            st[sp++] = Frame{f.lo, n2, 0.0, 0};
        } else if (f.state == 1) {
            f.left = ret;
            f.state = 2;
            st[sp++] = Frame{f.lo + n2, f.n - n2, 0.0, 0};
        } else {
            ret = f.left + ret;
            --sp;
        }
    }
    return ret;
}

// np.sum of a column of n elements
template <class LeafSum>
M6A_HD inline double colsum_by(LeafSum &&leaf_sum, int64_t n)
{
    if (n <= 0) return 0.0;
    double acc = pairwise(leaf_sum, 0, n < kPiece ? n : kPiece);
    for (int64_t at = kPiece; at < n; at += kPiece) acc += pairwise(leaf_sum, at, n - at < kPiece ? n - at : kPiece);
    return acc;
}

template <class Get>
M6A_HD inline double colsum(Get &&get, int64_t n)
{
    return colsum_by([&](int64_t lo, int64_t k) { return leaf(get, lo, k); }, n);
}

// the factors of one 5-mer and column from its sums over N reads
M6A_HD inline void finish(double S, double S2, int64_t N, double *mean, double *sd)
{
    const double n = (double)N, m = S / n, q = S2 / n, mm = m * m;
    *mean = m;
    *sd = sqrt(q - mm);
}

}  // namespace m6a_norm
#endif  // M6A_NORM_H

#if defined(M6A_NORM_DEVICE_PART) && !defined(M6A_NORM_DEVICE_PART_DONE)
#define M6A_NORM_DEVICE_PART_DONE
// ---- part 2: the kernels and m6a_norm_factors_build; in m6a_prep.hip behind m6a_json.h, whose scan and row walk it shares ---------
//   norm_scan_kernel   json_scan_site per site (one wave): the header, the 7-mer, the row starts.  No table is looked up.
//   norm_rows_kernel   json_rows_site, a lane per row: the nine raw doubles of every row to V [R][9].
//   norm_sums_kernel   one workgroup per site, 144 lanes: (values | squares) x nine columns x the eight accumulators of a leaf.  A
//                      lane owns one accumulator chain; the eight of a leaf meet in three xor steps, which add the pairs colsum adds
//                      (an IEEE sum does not depend on the order of its two operands); the tail of a leaf, the tree above the leaves
//                      and the pieces are colsum_by's own text, walked by all eight lanes alike.
//   fold               entry e = 3 site + c keyed by its 5-mer, the radix passes (stable), heads, one lane per (5-mer, values |
//                      squares, column) down its entries in order; N in int64.
// Declined sites: the host half's partials are copied to their place before the fold.  The finish runs on the host from the sums.
namespace {

using namespace m6a_json;

__global__ void __launch_bounds__(kBlk)
norm_scan_kernel(const uint8_t *__restrict__ f, const JsonSite *__restrict__ sites, const int64_t *__restrict__ off, int64_t S,
                 const uint8_t *__restrict__ blob, const int64_t *__restrict__ tx_off, int32_t *__restrict__ row_start,
                 uint64_t *__restrict__ site_k7, uint8_t *__restrict__ status)
{
    const int lane = (int)(threadIdx.x & 63);
    const int64_t s = (int64_t)blockIdx.x * kJsonWaves + (threadIdx.x >> 6);
    if (s >= S) return;
    const JsonSite st = sites[s];
    const int64_t base = off[s];
    uint64_t k7 = 0;
    const int reason = json_scan_site(f, st, base, off[s + 1] - base, lane, blob, tx_off, row_start, &k7);
    if (lane == 0) {
        status[s] = (uint8_t)reason;
        site_k7[s] = reason ? 0 : k7;
    }
}

struct NormSink {
    double *v;
    __device__ void operator()(int j, double x) const { if (j < 9) v[j] = x; }
};

__global__ void __launch_bounds__(kBlk)
norm_rows_kernel(const uint8_t *__restrict__ f, const JsonSite *__restrict__ sites, const int64_t *__restrict__ off, int64_t S,
                 const int32_t *__restrict__ row_start, double *__restrict__ V, uint8_t *status)
{
    const int lane = (int)(threadIdx.x & 63);
    const int64_t s = (int64_t)blockIdx.x * kJsonWaves + (threadIdx.x >> 6);
    if (s >= S || status[s]) return;
    const JsonSite st = sites[s];
    const int64_t base = off[s];
    const int r0 = json_rows_site(f, st, base, off[s + 1] - base, lane, row_start, [&](int64_t r) { return NormSink{V + 9 * (base + r)}; });
    if (r0 && lane == 0) status[s] = (uint8_t)r0;
}

constexpr int kNormLanes = 2 * 9 * 8;
static_assert(kNormLanes <= kBlk, "norm_sums_kernel: a workgroup holds a site's 144 chains");

__global__ void __launch_bounds__(kBlk)
norm_sums_kernel(const double *__restrict__ V, const int64_t *__restrict__ off, const uint8_t *__restrict__ status, double *__restrict__ s,
                 double *__restrict__ s2)
{
    const int64_t site = blockIdx.x;
    const int t = (int)threadIdx.x;
    if (t >= kNormLanes || status[site]) return;
    const int q = t / 72, j = (t % 72) >> 3, a = t & 7;         // the eight lanes of a (q, j) are neighbours in one wave
    const int64_t base = off[site], n = off[site + 1] - base;
    const double *const col = V + 9 * base + j;
    auto get = [&](int64_t r) {
        const double x = col[9 * r];
        return q ? x * x : x;
    };
    const double sum = m6a_norm::colsum_by([&](int64_t lo, int64_t k) {
        if (k < 8) return m6a_norm::leaf(get, lo, k);
        double r = get(lo + a);
        int64_t i;
        for (i = 8; i < k - k % 8; i += 8) r += get(lo + i + a);
        r += __shfl_xor(r, 1, 64);                               // r0 + r1, r2 + r3, r4 + r5, r6 + r7
        r += __shfl_xor(r, 2, 64);                               // (r0 + r1) + (r2 + r3), (r4 + r5) + (r6 + r7)
        r += __shfl_xor(r, 4, 64);
        for (; i < k; i++) r += get(lo + i);
        return r;
    }, n);
    if (a == 0) (q ? s2 : s)[9 * site + j] = sum;
}

__global__ void norm_key_kernel(const uint64_t *__restrict__ site_k7, int64_t E, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const int64_t e = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (e >= E) return;
    key[e] = kmer5_of(site_k7[e / 3], (int)(e % 3));
    val[e] = (uint32_t)e;
}

__global__ void norm_head_kernel(const uint64_t *__restrict__ key, int64_t E, int64_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x;
    if (i < E) flag[i] = i == 0 || key[i] != key[i - 1];
}

struct NormRec { uint64_t key; int64_t N; double S[3], S2[3]; };

// lane (k, w): w = 0..2 the columns of the values, 3..5 of the squares; the chain starts from the first entry's sum
__global__ void norm_fold_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, const uint32_t *__restrict__ seg, int64_t K,
                                 int64_t E, const int64_t *__restrict__ off, const double *__restrict__ s, const double *__restrict__ s2,
                                 NormRec *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * kBlk + threadIdx.x, k = g / 6;
    if (k >= K) return;
    const int w = (int)(g % 6), j = w % 3;
    const int64_t i0 = seg[k], i1 = k + 1 < K ? (int64_t)seg[k + 1] : E;
    const double *const src = w < 3 ? s : s2;
    double acc = 0.0;
    int64_t N = 0;
    // the additions are one chain in list order; the loads of sixteen entries are issued together, ahead of their additions
    constexpr int kAhead = 16;
    for (int64_t i = i0; i < i1; i += kAhead) {
        const int m = (int)(i1 - i < kAhead ? i1 - i : kAhead);
        double x[kAhead];
        int64_t nr[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; u++)
            if (u < m) {
                const int64_t e = val[i + u], site = e / 3;
                x[u] = src[9 * site + 3 * (e % 3) + j];
                nr[u] = off[site + 1] - off[site];
            }
#pragma unroll
        for (int u = 0; u < kAhead; u++)
            if (u < m) {
                acc = i + u == i0 ? x[u] : acc + x[u];
                N += nr[u];
            }
    }
    (w < 3 ? out[k].S : out[k].S2)[j] = acc;
    if (w == 0) { out[k].key = key[i0]; out[k].N = N; }
}

int norm_impl(int device_id, const char *json_path, int64_t S, const char *tx_blob, const int64_t *tx_off, const int64_t *pos, const int64_t *start,
              const int64_t *end, const int64_t *n_reads, const m6a_norm_host_half *host, int n_threads, std::vector<NormRec> &recs,
              uint8_t *status_out, char *kmer7_out, m6a_norm_stats &I)
{
    const double t_all = now_ms();
    g_d2h = 0;
    int rc;
    auto host_fail = [&](int hrc) {
        const int code = hrc == -2 ? M6A_ENOMEM : hrc == -3 ? M6A_EIO : hrc == -4 ? M6A_EFORMAT : hrc == -1 ? M6A_EINVAL : M6A_EIO;
        const std::string text = host->error ? host->error() : "the host half failed";
        return prep_fail(code, "%s", text.c_str());
    };

    // ---- the host: the file's size, the site table
    Fd fd;
    fd.fd = ::open(json_path, O_RDONLY);
    if (fd.fd < 0) return prep_fail(M6A_EIO, "cannot open %s", json_path);
    struct stat stt;
    if (fstat(fd.fd, &stt) != 0) return prep_fail(M6A_EIO, "cannot stat %s", json_path);
    const int64_t n = (int64_t)stt.st_size;
    std::vector<int64_t> off((size_t)S + 1, 0);
    std::vector<JsonSite> hs((size_t)S);
    for (int64_t i = 0; i < S; i++) {
        if (n_reads[i] < 0 || tx_off[i + 1] < tx_off[i]) return prep_fail(M6A_EINVAL, "site table: row %lld", (long long)i);
        const bool ok = start[i] >= 0 && end[i] <= n && start[i] < end[i] && end[i] - start[i] < 0x7fffffffll;
        // a row is 21 bytes at the least: a count the range cannot hold gets no rows here, is declined ("count") and is the host's error
        off[(size_t)i + 1] = off[(size_t)i] + (ok && n_reads[i] <= (end[i] - start[i]) / 21 ? n_reads[i] : 0);
        hs[(size_t)i] = JsonSite{ok ? start[i] : 0, ok ? end[i] : 0, pos[i], (uint32_t)i, 0};       // not ok: declined as "range"
    }
    const int64_t R = off[(size_t)S], E = 3 * S, blob_len = tx_off[S];

    // ---- device memory, all of it under the budget before a byte goes up
    DevMem m;
    if ((rc = open_device(device_id, m, "run `compute_norm_factors --device cpu`, which sums on the host"))) return rc;
    uint8_t *df, *dblob, *dstatus;
    JsonSite *dsites;
    int64_t *doff, *dtx_off, *flag;
    int32_t *row_start;
    uint64_t *site_k7, *key, *key2;
    uint32_t *val, *val2, *seg;
    double *V, *ds, *ds2;
    if ((rc = m.alloc(df, (size_t)padded(n), "data.json")) || (rc = m.alloc(dsites, (size_t)S, "the site table")) ||
        (rc = m.alloc(doff, (size_t)S + 1, "the offsets")) || (rc = m.alloc(dblob, (size_t)blob_len + 1, "transcript names")) ||
        (rc = m.alloc(dtx_off, (size_t)S + 1, "transcript names")) || (rc = m.alloc(row_start, (size_t)R + 1, "row starts")) ||
        (rc = m.alloc(site_k7, (size_t)S, "7-mers")) || (rc = m.alloc(dstatus, (size_t)S, "the status bytes")) ||
        (rc = m.alloc(V, (size_t)R * 9, "the rows' values")) || (rc = m.alloc(ds, (size_t)S * 9, "site sums")) ||
        (rc = m.alloc(ds2, (size_t)S * 9, "site sums")) || (rc = m.alloc(key, (size_t)E, "entries")) || (rc = m.alloc(key2, (size_t)E, "entries")) ||
        (rc = m.alloc(val, (size_t)E, "entries")) || (rc = m.alloc(val2, (size_t)E, "entries")) || (rc = m.alloc(flag, (size_t)E + 1, "entries")) ||
        (rc = m.alloc(seg, (size_t)E, "entries")))
        return rc;

    // ---- upload: data.json whole through the pinned pair; the table goes up beside it
    Streams St;
    int64_t chunk = 0;
    if ((rc = St.open(padded(n), chunk))) return rc;
    hipStream_t s = St.s[0];
    double t1 = now_ms();
    if ((rc = h2d(dsites, hs.data(), (size_t)S, s)) || (rc = h2d(doff, off.data(), (size_t)S + 1, s)) ||
        (rc = h2d(dblob, (const uint8_t *)tx_blob, (size_t)blob_len, s)) || (rc = h2d(dtx_off, tx_off, (size_t)S + 1, s)) ||
        (rc = upload_range(device_id, fd.fd, json_path, St, df, 0, n, chunk)))
        return rc;
    PCHK(hipStreamSynchronize(s));
    I.ms_upload = now_ms() - t1;

    // ---- scan, rows, sums; a status byte and the 7-mer per site come back
    t1 = now_ms();
    std::vector<uint8_t> status((size_t)S);
    std::vector<uint64_t> k7((size_t)S);
    const unsigned blocks = (unsigned)((S + kJsonWaves - 1) / kJsonWaves);
    norm_scan_kernel<<<blocks, kBlk, 0, s>>>(df, dsites, doff, S, dblob, dtx_off, row_start, site_k7, dstatus);
    PCHK(hipGetLastError());
    norm_rows_kernel<<<blocks, kBlk, 0, s>>>(df, dsites, doff, S, row_start, V, dstatus);
    PCHK(hipGetLastError());
    norm_sums_kernel<<<(unsigned)S, kBlk, 0, s>>>(V, doff, dstatus, ds, ds2);
    PCHK(hipGetLastError());
    if ((rc = d2h(status.data(), dstatus, (size_t)S, s)) || (rc = d2h(k7.data(), site_k7, (size_t)S, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    I.ms_kernels = now_ms() - t1;

    // ---- declined sites, in ascending order through the host half: their partials to their place, or the loader's first error
    t1 = now_ms();
    std::vector<int64_t> decl;
    for (int64_t i = 0; i < S; i++)
        if (status[(size_t)i]) decl.push_back(i);
    if (!decl.empty()) {
        const size_t D = decl.size();
        std::vector<double> hs1(D * 9), hs2(D * 9);
        std::vector<char> h7(D * 7);
        const int hrc = host->partials(json_path, S, tx_blob, tx_off, pos, start, end, n_reads, decl.data(), (int64_t)D, n_threads, hs1.data(),
                                       hs2.data(), h7.data());
        if (hrc) return host_fail(hrc);
        for (size_t k = 0; k < D; k++) {
            const int64_t i = decl[k];
            uint64_t x = 0;
            for (int j = 0; j < 7; j++) x = x << 8 | (uint8_t)h7[7 * k + (size_t)j];
            k7[(size_t)i] = x;
            if ((rc = h2d(ds + 9 * i, hs1.data() + 9 * k, 9, s)) || (rc = h2d(ds2 + 9 * i, hs2.data() + 9 * k, 9, s)) ||
                (rc = h2d(site_k7 + i, &k7[(size_t)i], 1, s)))
                return rc;
        }
        PCHK(hipStreamSynchronize(s));
    }
    I.ms_host = now_ms() - t1;

    // ---- the fold
    t1 = now_ms();
    int64_t K = 0;
    if ((rc = launch(norm_key_kernel, E, s, site_k7, E, key, val)) || (rc = radix_sort(m, key, val, key2, val2, E, 40, s)) ||
        (rc = launch(norm_head_kernel, E, s, key, E, flag)) || (rc = scan_total(m, flag, E, s, K)) ||
        (rc = launch(compact_u32_kernel, E, s, flag, E, seg)))
        return rc;
    NormRec *drec;
    if ((rc = m.alloc(drec, (size_t)K, "the 5-mers' sums")) || (rc = launch(norm_fold_kernel, 6 * K, s, key, val, seg, K, E, doff, ds, ds2, drec))) return rc;
    recs.resize((size_t)K);
    if ((rc = d2h(recs.data(), drec, (size_t)K, s))) return rc;
    PCHK(hipStreamSynchronize(s));
    I.ms_fold = now_ms() - t1;

    for (int64_t i = 0; i < S; i++) {
        if (status_out) status_out[i] = status[(size_t)i];
        for (int j = 0; kmer7_out && j < 7; j++) kmer7_out[7 * i + j] = (char)(k7[(size_t)i] >> (8 * (6 - j)));
    }
    I.n_sites = S; I.n_reads = R; I.n_kmers = K; I.n_declined = (int64_t)decl.size();
    I.d2h_bytes = g_d2h;
    I.peak_bytes = (int64_t)m.peak;
    I.ms_total = now_ms() - t_all;
    return M6A_OK;
}

}  // namespace

extern "C" int m6a_norm_factors_build(int device_id, const char *json_path, int64_t n_sites, const char *tx_blob, const int64_t *tx_off,
                                      const int64_t *pos, const int64_t *start, const int64_t *end, const int64_t *n_reads,
                                      const m6a_norm_host_half *host, int n_threads, char *kmers, int64_t *N, double *S, double *S2, double *mean,
                                      double *sd, int64_t *n_kmers, uint8_t *status, char *kmer7, m6a_norm_stats *stats)
{
    if (!json_path || !n_kmers || n_sites < 0) return prep_fail(M6A_EINVAL, "null argument");
    *n_kmers = 0;
    if (!host || !host->partials) return prep_fail(M6A_EINVAL, "the host half is missing");
    if (n_sites > (1ll << 30)) return prep_fail(M6A_EINVAL, "more than 2^30 sites");
    if (n_sites && (!tx_blob || !tx_off || !pos || !start || !end || !n_reads || !kmers || !N || !S || !S2 || !mean || !sd))
        return prep_fail(M6A_EINVAL, "null argument");
    m6a_norm_stats I{};
    if (!n_sites) { if (stats) *stats = I; return M6A_OK; }
    const int rc = guarded([&] {
        std::vector<NormRec> recs;
        const int rc2 = norm_impl(device_id, json_path, n_sites, tx_blob, tx_off, pos, start, end, n_reads, host, n_threads, recs, status, kmer7, I);
        if (rc2) return rc2;
        for (size_t k = 0; k < recs.size(); k++) {                 // the radix passes leave the 5-mers in bytewise order
            const NormRec &r = recs[k];
            for (int j = 0; j < 5; j++) kmers[5 * k + (size_t)j] = (char)(r.key >> (8 * (4 - j)));
            N[k] = r.N;
            for (int j = 0; j < 3; j++) {
                S[3 * k + (size_t)j] = r.S[j];
                S2[3 * k + (size_t)j] = r.S2[j];
                m6a_norm::finish(r.S[j], r.S2[j], r.N, mean + 3 * k + (size_t)j, sd + 3 * k + (size_t)j);
            }
        }
        *n_kmers = (int64_t)recs.size();
        return (int)M6A_OK;
    });
    if (stats) *stats = I;
    return rc;
}
#endif  // M6A_NORM_DEVICE_PART
