// m6a_npy_write.h -- m6a_prep_sites_write_read_representation (include/m6a.h): data.read_representation.npy from the handle's
// device arrays, in rounds.  Included at the end of m6a_prep.hip, behind m6a_csv.h: it uses m6a_prep_kit.h (DevMem, Rounds,
// run_rounds, guarded) and the pwrite helpers and Account of m6a_csv.h; the header's bytes and the round rule are m6a_npy.h.
//
// Round k is whole sites [cut[k], cut[k + 1]) (m6a_npy::cut_rounds over the handle's host copy of off[]).  Two device buffers and
// two pinned buffers of the largest round are allocated before the first round and nothing after it.  Round k's kernels run on
// the context's stream (the round's CSR row rebased to 0, then enc_repr_kernel straight from X, site_kmers at their offsets in
// the handle's arrays) into device buffer k & 1; an event behind them lets the copy stream bring the round into pinned buffer
// k & 1; the host waits for that copy and pwrites the round at its offset.  Round k + 1 is queued before the host waits for
// round k's copy, so the copy of round k runs under the kernel of round k + 1 and the pwrite of round k - 1, and a buffer is
// reused only after the host has seen its copy complete and its pwrite return.
#include "m6a_npy.h"

namespace m6a_detail {                       // m6a_api.hip: the context's side
int repr_writer_begin(m6a_ctx *c, int device, hipStream_t *stream);
int repr_writer_round(m6a_ctx *c, const float *X, const uint8_t *km, const int64_t *off, int64_t *off_round, int64_t s0, int64_t s1,
                      int64_t r0, int64_t nr, void *repr, int dtype);
}  // namespace m6a_detail

namespace {

int repr_write_impl(m6a_prep_sites &P, m6a_ctx *ctx, const char *path, int dtype, int64_t n_limit, m6a_repr_write_stats &st)
{
    const m6a_prep_sites_info &I = P.info;
    if (dtype != M6A_REPR_F32 && dtype != M6A_REPR_F16) return prep_fail(M6A_EINVAL, "dtype %d is neither M6A_REPR_F32 nor M6A_REPR_F16", dtype);
    if (I.n_sites <= 0) return prep_fail(M6A_EINVAL, "the handle holds no site");
    const int64_t S = n_limit >= 0 ? std::min<int64_t>(n_limit, I.n_sites) : I.n_sites;
    const int64_t *off = I.off_host;
    const int64_t n_rows = off[S], rb = m6a_npy::row_bytes(dtype);

    DevMem m;
    int rc = open_device(P.device, m, nullptr);             // the advice is made below, when the rounds are known
    if (rc) return rc;
    hipStream_t s_ctx = nullptr;
    if ((rc = m6a_detail::repr_writer_begin(ctx, P.device, &s_ctx))) return prep_fail(rc, "%s", m6a_last_error(ctx));
    g_d2h = 0;
    Account<m6a_repr_write_stats> account{P, m, st};

    // ---- the rounds, and the four buffers of the largest one (the pinned pair counts against the budget like the device pair)
    const int64_t kb = round_kb("M6A_REPR_ROUND_KB", m6a_npy::kRoundKB);
    std::vector<int64_t> cut;
    const int64_t widest = m6a_npy::cut_rounds(off, S, kb << 10, dtype, cut);
    const int64_t n_rounds = (int64_t)cut.size() - 1, cap = std::max<int64_t>(widest * rb, 16);
    int64_t most_sites = 0;
    for (int64_t k = 0; k < n_rounds; k++) most_sites = std::max(most_sites, cut[(size_t)k + 1] - cut[(size_t)k]);
    char advice[160];
    snprintf(advice, sizeof advice, "set M6A_REPR_ROUND_KB below %lld (the largest round is %lld KB, and four buffers of it are held)",
             (long long)kb, (long long)((cap + 1023) >> 10));
    m.advice = advice;
    const int n_buf = n_rounds > 1 ? 2 : 1;
    Rounds rd;                               // s[0]: the copy stream of both rounds.  Events: kernel start, kernel end (the context's
                                             // stream); copy start, copy end
    char *dbuf[2] = {nullptr, nullptr};
    int64_t *doff[2] = {nullptr, nullptr};
    if (n_rows) {
        if (m.used + (size_t)(2 * n_buf) * (size_t)cap > m.budget)
            return prep_fail(M6A_ENOMEM, "the read representation's %d buffers of %lld KB need more than the budget of %zu MB: %s", 2 * n_buf,
                             (long long)((cap + 1023) >> 10), m.budget >> 20, advice);
        if ((rc = rd.open(4, 1))) return rc;
        for (int i = 0; i < n_buf; i++) {
            if ((rc = m.alloc(dbuf[i], (size_t)cap, "read representation")) || (rc = m.alloc(doff[i], (size_t)most_sites + 1, "round offsets")) ||
                (rc = rd.pinned(i, cap)))
                return rc;
            m.used += (size_t)cap;
            m.peak = std::max(m.peak, m.used);
        }
    }

    // ---- the file: truncated, sized once, header first
    const std::string head = m6a_npy::header(n_rows, dtype);
    const int64_t at0 = (int64_t)head.size();
    struct Unlink {                          // an error behind this point leaves no file
        const char *path; bool armed = true;
        ~Unlink() { if (armed) (void)::unlink(path); }
    };
    Fd f;
    f.fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (f.fd < 0) return prep_fail(M6A_EIO, "cannot open %s", path);
    Unlink gone{path};
    if (::ftruncate(f.fd, (off_t)(at0 + n_rows * rb)) != 0) return prep_fail(M6A_EIO, "cannot size %s to %lld bytes", path, (long long)(at0 + n_rows * rb));
    if (!csv_pwrite_all(f.fd, head.data(), at0, 0)) return prep_fail(M6A_EIO, "cannot write %s", path);
    const int nw = std::min(m6a_usable_cpus(), 8);

    hipStream_t copy = rd.s[0];
    auto queue = [&](int64_t k) -> int {
        const int i = (int)(k & 1);
        const int64_t a = cut[(size_t)k], b = cut[(size_t)k + 1], r0 = off[a], nr = off[b] - r0;
        PCHK(hipEventRecord(rd.e[i][0], s_ctx));
        const int rc2 = m6a_detail::repr_writer_round(ctx, I.X, I.site_kmers, I.off, doff[i], a, b, r0, nr, dbuf[i], dtype);
        if (rc2) return prep_fail(rc2, "%s", m6a_last_error(ctx));
        PCHK(hipEventRecord(rd.e[i][1], s_ctx));
        PCHK(hipStreamWaitEvent(copy, rd.e[i][1], 0));
        PCHK(hipEventRecord(rd.e[i][2], copy));
        if (nr) PCHK(hipMemcpyAsync(rd.pin[i], dbuf[i], (size_t)(nr * rb), hipMemcpyDeviceToHost, copy));
        g_d2h += nr * rb;
        PCHK(hipEventRecord(rd.e[i][3], copy));
        return M6A_OK;
    };
    auto finish = [&](int64_t k) -> int {
        const int i = (int)(k & 1);
        PCHK(hipEventSynchronize(rd.e[i][3]));
        float km = 0, cm = 0;
        PCHK(hipEventElapsedTime(&km, rd.e[i][0], rd.e[i][1]));
        PCHK(hipEventElapsedTime(&cm, rd.e[i][2], rd.e[i][3]));
        st.ms_kernel += km;
        st.ms_copy += cm;
        const int64_t r0 = off[cut[(size_t)k]], nr = off[cut[(size_t)k + 1]] - r0;
        const double t0 = now_ms();
        if (!csv_pwrite_threads(f.fd, rd.pin[i], nr * rb, at0 + r0 * rb, nw)) return prep_fail(M6A_EIO, "cannot write %s", path);
        st.ms_write += now_ms() - t0;
        return M6A_OK;
    };
    if (n_rows && (rc = run_rounds(n_rounds, queue, finish))) return rc;
    st.n_rounds = n_rows ? n_rounds : 0;
    st.n_rows = n_rows;
    st.bytes = at0 + n_rows * rb;
    st.round_bytes = cap;
    const int cf = ::close(f.fd);
    f.fd = -1;
    if (cf != 0) return prep_fail(M6A_EIO, "cannot close %s", path);
    gone.armed = false;
    return M6A_OK;
}

}  // namespace

extern "C" int m6a_prep_sites_write_read_representation(m6a_prep_sites *p, m6a_ctx *ctx, const char *path, int dtype, int64_t n_sites_limit,
                                                        m6a_repr_write_stats *stats)
{
    m6a_repr_write_stats st{};
    int rc;
    if (!p || !ctx || !path) {
        rc = prep_fail(M6A_EINVAL, "null argument");
    } else {
        rc = guarded([&] { return repr_write_impl(*p, ctx, path, dtype, n_sites_limit, st); });
    }
    if (stats) *stats = st;
    return rc;
}
