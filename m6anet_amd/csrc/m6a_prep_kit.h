// m6a_prep_kit.h -- the host-side toolkit of m6a_prep.hip's translation unit: errors (prep_fail, PCHK, guarded), the device and its
// memory under a budget (open_device, DevMem), streams and pinned chunks with the one upload loop (Streams, upload_range), scans and
// sorts, text back to the host in rounds (Rounds, run_rounds; the cut is m6a_rounds.h).  m6a_prep.hip includes it once at its top and
// the headers included at that file's end (m6a_bgzf.h ... m6a_norm.h) use it; not a file to compile on its own.
#pragma once

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
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "m6a.h"
#include "m6a_rounds.h"

namespace {

thread_local std::string g_prep_err;
thread_local int64_t g_d2h = 0;          // bytes copied device -> host by this thread's current call (m6a_prep_sites reports them)

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

inline unsigned grid(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + kBlk - 1) / kBlk); }

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
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

#define PCHK(x)                                                                                                            \
    do {                                                                                                                   \
        hipError_t e_ = (x);                                                                                               \
        if (e_ != hipSuccess) return prep_fail(M6A_EHIP, "%s: %s", #x, hipGetErrorString(e_));                             \
    } while (0)

// scratch of the window loop: one allocation (counted like any other) that every window bump-allocates from the start, so that no
// hipMalloc or hipFree runs between the kernels of a window; a window that needs more says how much and is done again
struct Arena {
    uint8_t *base = nullptr;
    size_t cap = 0, off = 0, need = 0;
};
constexpr int kArenaFull = 1;               // DevMem::alloc's answer then; never leaves front_windows

// device memory of one call, every allocation counted against the budget (open_device sets it)
struct DevMem {
    std::vector<std::pair<void *, size_t>> ptrs;
    size_t used = 0, budget = 0, peak = 0;
    bool budget_set = false;                     // the first file of a job sets it; what stays of earlier files counts against it
    const char *advice = "use --device cpu";     // what the budget error tells the user to do instead
    Arena *arena = nullptr;                      // set: alloc() takes from it (release() of such a pointer does nothing)
    ~DevMem() { for (auto &p : ptrs) (void)hipFree(p.first); }
    template <class T> int alloc(T *&p, size_t count, const char *what)
    {
        const size_t bytes = std::max<size_t>(16, count * sizeof(T));
        if (arena) {
            const size_t a = (bytes + 255) & ~(size_t)255;
            if (arena->off + a > arena->cap) { arena->need = std::max(arena->need, arena->off + a); return kArenaFull; }
            p = (T *)(arena->base + arena->off);
            arena->off += a;
            return M6A_OK;
        }
        if (used + bytes > budget)
            return prep_fail(M6A_ENOMEM, "dataprep on the device needs more than its budget of %zu MB (%s: %zu MB used, %zu MB more); "
                             "this file does not fit: %s", budget >> 20, what, used >> 20, bytes >> 20, advice);
        void *q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) return prep_fail(M6A_ENOMEM, "hipMalloc of %zu MB failed (%s); %s", bytes >> 20, what, advice);
        ptrs.emplace_back(q, bytes);
        used += bytes;
        peak = std::max(peak, used);
        p = (T *)q;
        return M6A_OK;
    }
    // hipFree everything allocated from entry `mark` of ptrs on, but `keep`
    void release_since(size_t mark, std::initializer_list<const void *> keep)
    {
        std::vector<std::pair<void *, size_t>> left(ptrs.begin(), ptrs.begin() + (ptrdiff_t)std::min(mark, ptrs.size()));
        for (size_t i = mark; i < ptrs.size(); i++) {
            if (std::find(keep.begin(), keep.end(), (const void *)ptrs[i].first) != keep.end()) { left.push_back(ptrs[i]); continue; }
            (void)hipFree(ptrs[i].first);
            used -= ptrs[i].second;
        }
        ptrs.swap(left);
    }
    // hipFree now (release) or never (detach: the caller owns it from here on)
    void drop(const void *p, bool free_it)
    {
        for (size_t i = 0; i < ptrs.size(); i++)
            if (ptrs[i].first == p) {
                if (free_it) { (void)hipFree(ptrs[i].first); used -= ptrs[i].second; }
                ptrs.erase(ptrs.begin() + (ptrdiff_t)i);
                return;
            }
    }
    void release(const void *p) { drop(p, true); }
    void release(std::initializer_list<const void *> ps) { for (const void *p : ps) drop(p, true); }
    void detach(const void *p) { drop(p, false); }
    size_t size_of(const void *p) const
    {
        for (const auto &q : ptrs)
            if (q.first == p) return q.second;
        return 0;
    }
};

struct Streams {
    hipStream_t s[2] = {nullptr, nullptr};
    hipEvent_t copied[2] = {nullptr, nullptr};
    void *pin[2] = {nullptr, nullptr};
    // the two streams (s[0] kernels, s[1] copies), their events and the two pinned chunks: M6A_PREP_CHUNK_KB (default 64 MB) rounded up
    // to whole scan blocks and at most `most` bytes; `chunk` receives the size
    int open(int64_t most, int64_t &chunk)
    {
        for (int i = 0; i < 2; i++) {
            PCHK(hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking));
            PCHK(hipEventCreateWithFlags(&copied[i], hipEventDisableTiming));
        }
        const char *ck = getenv("M6A_PREP_CHUNK_KB");
        chunk = (ck && atoll(ck) > 0 ? atoll(ck) : 65536) << 10;
        chunk = std::max<int64_t>(kScanBytes, (chunk + kScanBytes - 1) / kScanBytes * kScanBytes);
        chunk = std::min<int64_t>(chunk, most);
        for (int i = 0; i < 2; i++) PCHK(hipHostMalloc(&pin[i], (size_t)chunk, hipHostMallocDefault));
        return M6A_OK;
    }
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

// the device of a call and, unless an earlier file of the job has set it, the budget of its DevMem: free memory minus a margin of a
// sixteenth (4 GB at most), or fewer MB if the environment says so.  advice: what the budget error tells the user to do instead (null: as it is)
int open_device(int device_id, DevMem &m, const char *advice)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return prep_fail(M6A_ENODEV, "no HIP device");
    if (device_id < 0 || device_id >= ndev) return prep_fail(M6A_EINVAL, "device %d of %d", device_id, ndev);
    PCHK(hipSetDevice(device_id));
    if (advice) m.advice = advice;
    if (m.budget_set) return M6A_OK;
    m.budget_set = true;
    size_t fr = 0, tot = 0;
    PCHK(hipMemGetInfo(&fr, &tot));
    const size_t margin = std::min<size_t>(fr / 16, (size_t)4 << 30);
    m.budget = fr > margin ? fr - margin : 0;
    const char *b = getenv("M6A_PREP_BUDGET_MB");
    if (b && atoll(b) > 0) m.budget = std::min(m.budget, (size_t)atoll(b) << 20);
    return M6A_OK;
}

// an extern "C" body: what it throws becomes a code and a text
template <class Body> int guarded(Body body)
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return prep_fail(M6A_ENOMEM, "out of host memory");
    } catch (...) {
        return prep_fail(M6A_EIO, "unexpected exception");
    }
}

struct Fd {
    int fd = -1;
    bool own = true;                        // false: descriptor 0 for `-`, which stays the process's
    ~Fd() { if (own && fd >= 0) ::close(fd); }
};

// one lane per item: grid(n) blocks of kBlk on s, and nothing at n <= 0
template <class... P, class... A> int launch(void (*kernel)(P...), int64_t n, hipStream_t s, A... args)
{
    if (n <= 0) return M6A_OK;
    kernel<<<grid(n), kBlk, 0, s>>>(args...);
    PCHK(hipGetLastError());
    return M6A_OK;
}

// len rounded up to whole scan blocks, one at the least: what a text buffer holds, zeros behind the text
inline int64_t padded(int64_t len) { return std::max<int64_t>(1, (len + kScanBytes - 1) / kScanBytes) * kScanBytes; }

// one value device -> host, there when this returns
template <class T> int fetch(T &host, const T *dev, hipStream_t s)
{
    PCHK(hipMemcpyAsync(&host, dev, sizeof(T), hipMemcpyDeviceToHost, s));
    g_d2h += (int64_t)sizeof(T);
    PCHK(hipStreamSynchronize(s));
    return M6A_OK;
}

// file bytes [off, off + len) -> dst, all of them
int read_fully(int fd, void *dst, int64_t len, int64_t off, const char *path)
{
    for (int64_t got = 0; got < len;) {
        const ssize_t r = ::pread(fd, (char *)dst + got, (size_t)(len - got), (off_t)(off + got));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return prep_fail(M6A_EIO, "cannot read %s", path);
        got += r;
    }
    return M6A_OK;
}

int write_fully(int fd, const void *src, size_t len, const char *path)
{
    for (size_t got = 0; got < len;) {
        const ssize_t k = ::write(fd, (const char *)src + got, len - got);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) return prep_fail(M6A_EIO, "cannot write %s", path);
        got += (size_t)k;
    }
    return M6A_OK;
}

// names -> ids in order of first appearance; a new name goes behind blob, where tx_off says it starts (the caller closes tx_off)
struct Interner {
    std::string &blob;
    std::vector<int64_t> &tx_off;
    std::unordered_map<std::string, uint32_t> ids;
    Interner(std::string &b, std::vector<int64_t> &o) : blob(b), tx_off(o) {}
    uint32_t id(const std::string &nm)
    {
        auto it = ids.find(nm);
        if (it != ids.end()) return it->second;
        const uint32_t t = (uint32_t)ids.size();
        ids.emplace(nm, t);
        tx_off.push_back((int64_t)blob.size());
        blob += nm;
        return t;
    }
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
    return rc ? rc : fetch(total, a + n, s);
}

constexpr int kUploadStop = 2;              // a per_chunk hook's answer that ends upload_range without an error; never leaves it

// file bytes [off, off + len) -> dst on the copy stream, zeros behind them to a whole scan block (pad; a buffer of exactly len bytes
// takes none); returns when they have arrived.
// per_chunk(slot, done, part) is called when the copy of bytes [done, done + part) has been recorded as S.copied[slot], while
// S.pin[slot] still holds them: the resident file counts the chunk's newlines behind that event while the next chunk is read (the
// zeros go first, so the last block is whole then)
template <class Hook>
int upload_range(int device_id, int fd, const char *path, Streams &S, uint8_t *dst, int64_t off, int64_t len, int64_t chunk, Hook per_chunk,
                 bool pad = true)
{
    int rc;
    PCHK(hipSetDevice(device_id));
    if (pad && padded(len) > len) PCHK(hipMemsetAsync(dst + len, 0, (size_t)(padded(len) - len), S.s[1]));
    for (int64_t k = 0, done = 0; done < len; k++, done += chunk) {
        const int slot = (int)(k & 1);
        PCHK(hipEventSynchronize(S.copied[slot]));          // the copy that last used this buffer is done
        const int64_t part = std::min(chunk, len - done);
        if ((rc = read_fully(fd, S.pin[slot], part, off + done, path))) return rc;
        PCHK(hipMemcpyAsync(dst + done, S.pin[slot], (size_t)part, hipMemcpyHostToDevice, S.s[1]));
        PCHK(hipEventRecord(S.copied[slot], S.s[1]));
        if ((rc = per_chunk(slot, done, part)) == kUploadStop) break;
        if (rc) return rc;
    }
    PCHK(hipStreamSynchronize(S.s[1]));
    return M6A_OK;
}

int upload_range(int device_id, int fd, const char *path, Streams &S, uint8_t *dst, int64_t off, int64_t len, int64_t chunk)
{
    return upload_range(device_id, fd, path, S, dst, off, len, chunk, [](int, int64_t, int64_t) { return M6A_OK; });
}

constexpr int kRadixItems = 16, kRadixTile = kBlk * kRadixItems;     // 4096 keys per block
static_assert(kBlk == 256, "radix_scatter_kernel scans 16 digits x 16 chunks of 16 lanes: one lane per (digit, chunk)");

__global__ void radix_hist_kernel(const uint64_t *__restrict__ key, int64_t n, int shift, int64_t nblk, int64_t *__restrict__ hist)
{
    __shared__ int c[16];
    if (threadIdx.x < 16) c[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kRadixTile;
    for (int k = 0; k < kRadixItems; k++) {
        const int64_t i = base + (int64_t)k * kBlk + threadIdx.x;
        if (i < n) atomicAdd(&c[(key[i] >> shift) & 15], 1);
    }
    __syncthreads();
    if (threadIdx.x < 16) hist[threadIdx.x * nblk + blockIdx.x] = c[threadIdx.x];
}

// stable: lane t owns keys [16 t, 16 t + 16) of the block's tile, in order; hist = exclusive scan, digit-major then block
__global__ void radix_scatter_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, int64_t n, int shift, int64_t nblk,
                                     const int64_t *__restrict__ hist, uint64_t *__restrict__ key2, uint32_t *__restrict__ val2)
{
    __shared__ int cnt[16][kBlk];
    __shared__ int part[16][16];
    const int t = threadIdx.x;
    for (int d = 0; d < 16; d++) cnt[d][t] = 0;
    const int64_t i0 = (int64_t)blockIdx.x * kRadixTile + (int64_t)t * kRadixItems;
    for (int k = 0; k < kRadixItems; k++)
        if (i0 + k < n) cnt[(key[i0 + k] >> shift) & 15][t]++;
    __syncthreads();
    const int d = t >> 4, c = t & 15;                  // per digit, the exclusive scan over the lanes: 16 chunks of 16 lanes
    int sum = 0;
    for (int k = 0; k < 16; k++) sum += cnt[d][c * 16 + k];
    part[d][c] = sum;
    __syncthreads();
    if (t < 16) {
        int run = 0;
        for (int k = 0; k < 16; k++) { const int v = part[t][k]; part[t][k] = run; run += v; }
    }
    __syncthreads();
    int run = part[d][c];
    for (int k = 0; k < 16; k++) { const int v = cnt[d][c * 16 + k]; cnt[d][c * 16 + k] = run; run += v; }
    __syncthreads();
    for (int k = 0; k < kRadixItems && i0 + k < n; k++) {
        const uint64_t x = key[i0 + k];
        const int g = (int)((x >> shift) & 15);
        const int64_t o = hist[g * nblk + blockIdx.x] + cnt[g][t]++;
        key2[o] = x;
        val2[o] = val[i0 + k];
    }
}

// stable sort of (key, val) by the low `bits` bits of key; key / val end up pointing at the sorted pair (swapped with key2 / val2)
int radix_sort(DevMem &m, uint64_t *&key, uint32_t *&val, uint64_t *&key2, uint32_t *&val2, int64_t n, int bits, hipStream_t s)
{
    if (n <= 1 || bits <= 0) return M6A_OK;
    const int64_t nblk = (n + kRadixTile - 1) / kRadixTile;
    int64_t *hist;
    int rc = m.alloc(hist, (size_t)(16 * nblk) + 1, "sort");
    if (rc) return rc;
    for (int sh = 0; sh < bits; sh += 4) {
        radix_hist_kernel<<<(unsigned)nblk, kBlk, 0, s>>>(key, n, sh, nblk, hist);
        PCHK(hipGetLastError());
        if ((rc = scan_excl(m, hist, 16 * nblk, s))) return rc;
        radix_scatter_kernel<<<(unsigned)nblk, kBlk, 0, s>>>(key, val, n, sh, nblk, hist, key2, val2);
        PCHK(hipGetLastError());
        std::swap(key, key2);
        std::swap(val, val2);
    }
    PCHK(hipStreamSynchronize(s));
    m.release(hist);
    return M6A_OK;
}

// stable sort of (key, val) by up to three fields, given by their bit widths, least significant first.  As many fields as fit into
// 64 bits go into one key: make_key(use, shift) launches the caller's key kernel for the fields whose bit is set in `use`, field f at
// bit shift[f], and radix_sort sorts by what was packed; the fields that are left follow in further passes (LSD, stable).
template <class MakeKey>
int sort_by_fields(DevMem &m, hipStream_t s, const int *bits, int n_fields, uint64_t *&key, uint32_t *&val, uint64_t *&key2, uint32_t *&val2, int64_t n,
                   MakeKey make_key)
{
    int rc, shift[3] = {0, 0, 0}, at = 0;
    unsigned use = 0;
    for (int f = 0; f <= n_fields; f++) {
        if (f == n_fields || (bits[f] && at + bits[f] > 64)) {          // sort by what is packed so far
            if (use && ((rc = make_key(use, shift)) || (rc = radix_sort(m, key, val, key2, val2, n, at, s)))) return rc;
            use = 0;
            at = 0;
        }
        if (f == n_fields || !bits[f]) continue;
        shift[f] = at;
        use |= 1u << f;
        at += bits[f];
    }
    return M6A_OK;
}

template <class T> int d2h(T *dst, const T *src, size_t count, hipStream_t s)
{
    if (!count) return M6A_OK;
    PCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, s));
    g_d2h += (int64_t)(count * sizeof(T));
    return M6A_OK;
}

template <class T> int h2d(T *dst, const T *src, size_t count, hipStream_t s)
{
    if (!count) return M6A_OK;
    PCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, s));
    return M6A_OK;
}

// the 66-word vocabulary of m6a_io.cpp (sorted unique 5-mers of all N-DRACH-N 7-mers), packed like pack5
std::vector<uint64_t> vocab_keys()
{
    std::vector<uint64_t> v;
    const std::string N = "ACGT", D = "AGT", R = "GA", H = "ACT";
    for (char a : N) for (char d : D) for (char r : R) for (char h : H) for (char b : N) {
        const char k7[7] = {a, d, r, 'A', 'C', h, b};
        for (int i = 0; i < 3; i++) {
            uint64_t x = 0;
            for (int j = 0; j < 5; j++) x = x << 8 | (uint8_t)k7[i + j];
            v.push_back(x);
        }
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

// ---- text back in rounds: two rounds in flight, each with a stream, events and a pinned buffer --------------------------------------
// M6A_*_ROUND_KB as a number of KB (unset, 0 or not a number: dflt)
inline int64_t round_kb(const char *env_name, int64_t dflt)
{
    const char *e = getenv(env_name);
    return e && atoll(e) > 0 ? atoll(e) : dflt;
}

struct Rounds {                             // round k uses slot k & 1
    hipStream_t s[2] = {nullptr, nullptr};
    hipEvent_t e[2][6] = {};                // what each of them brackets is the writer's to say
    char *pin[2] = {nullptr, nullptr};
    int open(int n_events, int n_streams = 2)
    {
        for (int i = 0; i < n_streams; i++) PCHK(hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking));
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < n_events; j++) PCHK(hipEventCreate(&e[i][j]));
        return M6A_OK;
    }
    int pinned(int slot, int64_t bytes)
    {
        PCHK(hipHostMalloc((void **)&pin[slot], (size_t)std::max<int64_t>(bytes, 16), hipHostMallocDefault));
        return M6A_OK;
    }
    ~Rounds()                               // nothing is freed under a copy in flight
    {
        for (hipStream_t x : s) if (x) (void)hipStreamSynchronize(x);
        for (auto &ev : e) for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
        for (char *x : pin) if (x) (void)hipHostFree(x);
        for (hipStream_t x : s) if (x) (void)hipStreamDestroy(x);
    }
};

// Round k + 1 is queued before the host waits for round k: queue(k) puts a round's kernels and copy on its stream, finish(k) waits for
// its last event, adds its event times to the statistics and pwrites it.  settle(k) is what must happen to round k before round
// k + 1 may be queued: nothing, except in the BGZF writer, which learns the size of the payload copy from the round's status words.
template <class Queue, class Settle, class Finish> int run_rounds(int64_t n_rounds, Queue queue, Settle settle, Finish finish)
{
    int rc;
    if (n_rounds && (rc = queue(0))) return rc;
    for (int64_t k = 0; k < n_rounds; k++) {
        if ((rc = settle(k))) return rc;
        if (k + 1 < n_rounds && (rc = queue(k + 1))) return rc;
        if ((rc = finish(k))) return rc;
    }
    return M6A_OK;
}

template <class Queue, class Finish> int run_rounds(int64_t n_rounds, Queue queue, Finish finish)
{
    return run_rounds(n_rounds, queue, [](int64_t) { return M6A_OK; }, finish);
}

// the normalisation 5-mers packed like pack5, sorted, each once: keys, and per key the index of the first of equal 5-mers (the
// loader's map keeps the first)
void norm_keys(const char *norm_kmers, int n_norm, std::vector<uint64_t> &keys, std::vector<int32_t> &first)
{
    std::vector<std::pair<uint64_t, int32_t>> norm;
    for (int i = 0; i < n_norm; i++) {
        uint64_t x = 0;
        for (int j = 0; j < 5; j++) x = x << 8 | (uint8_t)norm_kmers[5 * i + j];
        norm.emplace_back(x, i);
    }
    std::sort(norm.begin(), norm.end());
    for (size_t i = 0; i < norm.size(); i++)
        if (i == 0 || norm[i].first != norm[i - 1].first) { keys.push_back(norm[i].first); first.push_back(norm[i].second); }
}

}  // namespace
