// pointer_convention_core_main.cpp -- the host-side checks of m6anet_amd/csrc/m6a_ctx.h (csr_check, same_side, enter) as a program of
// its own, for the sanitizers: tests/test_pointer_convention_core.py builds it with hipcc, host pass only, under
// -fsanitize=address,undefined and runs it as a child process.  No HIP call is made: is_device_ptr, fail and job_busy, which the
// library defines in m6a_api.hip, are stood in for here -- a pointer is a "device pointer" when it points into `device_side`.
//
// Every off[] is a heap allocation of exactly S + 1 entries, so a read past the array is a sanitizer report.  One line per case,
// "ok <case>" or "FAILED <case>: ..."; the exit status is the number of failed cases.
#include "m6a_ctx.h"

static char device_side[64];

namespace m6a_detail {

bool is_device_ptr(const void *p) { return p >= (const void *)device_side && p < (const void *)(device_side + sizeof device_side); }

int fail(m6a_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->err = buf;
    return code;
}

int job_busy(m6a_ctx *c)
{
    if (c->job.open) return fail(c, M6A_EINVAL, "a streaming job is open on this context (m6a_job_end or m6a_job_abort first)");
    return M6A_OK;
}

}  // namespace m6a_detail

using namespace m6a_detail;

static int failed = 0;

static void expect(const char *what, m6a_ctx &c, int got, int want, const char *text)
{
    const bool ok = got == want && (want >= 0 || c.err == text);
    printf("%s %s", ok ? "ok" : "FAILED", what);
    if (!ok) printf(": returned %d \"%s\", expected %d \"%s\"", got, c.err.c_str(), want, text);
    printf("\n");
    failed += !ok;
    c.err.clear();
}

static int csr(m6a_ctx &c, std::initializer_list<int64_t> off)
{
    std::unique_ptr<int64_t[]> a(new int64_t[off.size()]);
    std::copy(off.begin(), off.end(), a.get());
    return csr_check(&c, a.get(), (int64_t)off.size() - 1);
}

int main()
{
    m6a_ctx c;
    const char *off0 = "off[0] must be 0", *decr = "off[] must be non-decreasing", *mixed = "a, b, c must be all host or all device pointers";
    expect("csr: no sites", c, csr(c, {0}), M6A_OK, "");
    expect("csr: bags 1 2 15 16 17 40", c, csr(c, {0, 1, 3, 18, 34, 51, 91}), M6A_OK, "");
    expect("csr: empty sites", c, csr(c, {0, 0, 5, 5, 5}), M6A_OK, "");
    expect("csr: off[0] = 1", c, csr(c, {1, 1, 3}), M6A_EINVAL, off0);
    expect("csr: off[0] = -1", c, csr(c, {-1, 1, 3}), M6A_EINVAL, off0);
    expect("csr: off[0] = 1 and no sites", c, csr(c, {1}), M6A_EINVAL, off0);
    expect("csr: a decreasing first step", c, csr(c, {0, -1}), M6A_EINVAL, decr);
    expect("csr: a decreasing last step", c, csr(c, {0, 1, 3, 2}), M6A_EINVAL, decr);
    expect("csr: the widest decreasing step", c, csr(c, {0, INT64_MAX, INT64_MIN}), M6A_EINVAL, decr);
    expect("csr: both faults, off[0] wins", c, csr(c, {2, 1}), M6A_EINVAL, off0);

    char host_side[64];
    const void *h0 = host_side, *h1 = host_side + 8, *d0 = device_side, *d1 = device_side + 8, *d2 = device_side + 63;
    expect("side: all host", c, same_side(&c, h0, {h1, h0}, mixed), 0, "");
    expect("side: all device", c, same_side(&c, d0, {d1, d2}, mixed), 1, "");
    expect("side: one pointer", c, same_side(&c, d0, {}, mixed), 1, "");
    expect("side: optional pointers left out", c, same_side(&c, h0, {h1, nullptr, nullptr}, mixed), 0, "");
    expect("side: device call, optional left out", c, same_side(&c, d0, {nullptr, d1}, mixed), 1, "");
    expect("side: first on the device", c, same_side(&c, d0, {h0, h1}, mixed), M6A_EINVAL, mixed);
    expect("side: last on the device", c, same_side(&c, h0, {h1, d0}, mixed), M6A_EINVAL, mixed);
    expect("side: an optional pointer on the other side", c, same_side(&c, d0, {d1, nullptr, h0}, mixed), M6A_EINVAL, mixed);
    expect("side: one past the device block is host", c, same_side(&c, d0, {device_side + sizeof device_side}, mixed), M6A_EINVAL, mixed);
    expect("side: a sentence with a per cent sign", c, same_side(&c, d0, {h0}, "100%s of %d"), M6A_EINVAL, "100%s of %d");

    expect("enter: no context", c, enter(nullptr), M6A_EINVAL, "");
    expect("enter: an idle context", c, enter(&c), M6A_OK, "");
    c.job.open = true;
    expect("enter: a streaming job is open", c, enter(&c), M6A_EINVAL, "a streaming job is open on this context (m6a_job_end or m6a_job_abort first)");
    c.job.open = false;
    {
        HintScope scope(&c);
        c.hint_off = (const int64_t *)host_side;
    }
    expect("hint scope: the hint is consumed on the way out", c, c.hint_off == nullptr, 1, "");
    return failed;
}
