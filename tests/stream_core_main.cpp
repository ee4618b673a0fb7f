// The stream reader core (m6anet_amd/csrc/m6a_stream.h) as a program of its own: tests/test_stream_core.py builds it with ASan and
// UBSan and runs it.  A writer thread delivers a seeded buffer through a real pipe() in pieces of a given size (0: random sizes), the
// reader fills requests of a given size, and the program prints one line per case: `ok <bytes>` or what went wrong.
//   stream_core <seed> <bytes> pieces <piece> <request>     the buffer comes back byte for byte, at_eof() is 0 before every request
//                                                           that still has a byte to get and 1 exactly after the last byte
//   stream_core <seed> <bytes> ring <piece> <request> <buffer>   the same through the read-ahead ring with two buffers of <buffer> bytes:
//                                                           requests end in the middle of a buffer, on its last byte and behind it
//   stream_core <seed> <bytes> abandon <piece> <buffer>     the ring is left while the writer still writes: nothing waits for the rest
//   stream_core <seed> <bytes> empty                        a pipe nobody wrote to is at its end at once
//   stream_core <seed> <bytes> closed                       a closed descriptor: fill and at_eof are -1, the text names the path
#include <errno.h>
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "m6a_stream.h"

namespace {

void write_all(int fd, const uint8_t *p, size_t n)
{
    while (n > 0) {
        const ssize_t r = ::write(fd, p, n);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return;                                  // the reader went away: it reports what it missed
        p += r;
        n -= (size_t)r;
    }
}

int pieces(const std::vector<uint8_t> &data, uint64_t seed, int64_t piece, int64_t request)
{
    int fds[2];
    if (pipe(fds) != 0) { printf("pipe failed\n"); return 1; }
    std::thread writer([&data, seed, piece, wfd = fds[1]]() {
        std::mt19937_64 rng(seed ^ 0x9e3779b97f4a7c15ull);
        for (size_t at = 0; at < data.size();) {
            const size_t k = std::min<size_t>(data.size() - at, piece > 0 ? (size_t)piece : (size_t)(1 + rng() % 9000));
            write_all(wfd, data.data() + at, k);
            at += k;
        }
        ::close(wfd);
    });
    int bad = 0;
    {
        m6a_stream::Reader R(fds[0], true, "the pipe");
        // the exact size: a read past the request's end is ASan's to find
        std::vector<uint8_t> buf((size_t)request);
        int64_t at = 0;
        const int64_t n = (int64_t)data.size();
        while (!bad) {
            const int e = R.at_eof();
            if (e != (at == n ? 1 : 0)) { printf("at_eof is %d at byte %lld of %lld\n", e, (long long)at, (long long)n); bad = 1; break; }
            if (at == n) break;
            const int64_t got = R.fill(buf.data(), request);
            if (got != std::min(request, n - at)) { printf("fill gave %lld at byte %lld\n", (long long)got, (long long)at); bad = 1; break; }
            if (memcmp(buf.data(), data.data() + at, (size_t)got) != 0) { printf("other bytes at %lld\n", (long long)at); bad = 1; break; }
            at += got;
            if (R.consumed != at) { printf("consumed is %lld at byte %lld\n", (long long)R.consumed, (long long)at); bad = 1; }
        }
        if (!bad && (R.fill(buf.data(), request) != 0 || R.at_eof() != 1)) { printf("bytes behind the end\n"); bad = 1; }
    }                                                        // the reader closes its end: a writer still writing gets EPIPE
    writer.join();
    if (!bad) printf("ok %lld\n", (long long)data.size());
    return bad;
}

std::thread writer_of(const std::vector<uint8_t> &data, uint64_t seed, int64_t piece, int wfd)
{
    return std::thread([&data, seed, piece, wfd]() {
        std::mt19937_64 rng(seed ^ 0x9e3779b97f4a7c15ull);
        for (size_t at = 0; at < data.size();) {
            const size_t k = std::min<size_t>(data.size() - at, piece > 0 ? (size_t)piece : (size_t)(1 + rng() % 9000));
            write_all(wfd, data.data() + at, k);
            at += k;
        }
        ::close(wfd);
    });
}

int ring(const std::vector<uint8_t> &data, uint64_t seed, int64_t piece, int64_t request, int64_t cap)
{
    int fds[2];
    if (pipe(fds) != 0) { printf("pipe failed\n"); return 1; }
    std::thread writer = writer_of(data, seed, piece, fds[1]);
    int bad = 0;
    {
        m6a_stream::Reader R(fds[0], true, "the pipe");
        std::vector<uint8_t> b0((size_t)cap), b1((size_t)cap), buf((size_t)request);
        m6a_stream::Ring ring(R, b0.data(), b1.data(), cap);
        ring.start();
        int64_t at = 0, settled = 0;
        const int64_t n = (int64_t)data.size();
        auto copy = [&](const uint8_t *p, int64_t k, int slot, int64_t off) {
            if (slot < 0 || slot > 1 || off + k > request) return false;
            memcpy(buf.data() + off, p, (size_t)k);
            return true;
        };
        auto settle = [&](int) { ++settled; return true; };
        while (!bad) {
            const int e = ring.at_eof();
            if (e != (at == n ? 1 : 0)) { printf("at_eof is %d at byte %lld of %lld\n", e, (long long)at, (long long)n); bad = 1; break; }
            if (at == n) break;
            const int64_t got = ring.take(request, copy, settle);
            if (got != std::min(request, n - at)) { printf("take gave %lld at byte %lld\n", (long long)got, (long long)at); bad = 1; break; }
            if (memcmp(buf.data(), data.data() + at, (size_t)got) != 0) { printf("other bytes at %lld\n", (long long)at); bad = 1; break; }
            at += got;
        }
        if (!bad && (ring.take(request, copy, settle) != 0 || ring.at_eof() != 1)) { printf("bytes behind the end\n"); bad = 1; }
        if (!bad && settled != std::max<int64_t>(1, (n + cap - 1) / cap)) {      // every buffer once, when its last byte was taken
            printf("%lld buffers settled\n", (long long)settled);
            bad = 1;
        }
    }
    writer.join();
    if (!bad) printf("ok %lld\n", (long long)data.size());
    return bad;
}

int abandon(const std::vector<uint8_t> &data, uint64_t seed, int64_t piece, int64_t cap)
{
    int fds[2];
    if (pipe(fds) != 0) { printf("pipe failed\n"); return 1; }
    std::thread writer = writer_of(data, seed, piece, fds[1]);
    int bad = 0;
    {
        m6a_stream::Reader R(fds[0], true, "the pipe");
        std::vector<uint8_t> b0((size_t)cap), b1((size_t)cap), buf(100);
        m6a_stream::Ring ring(R, b0.data(), b1.data(), cap);
        ring.start();
        auto copy = [&](const uint8_t *p, int64_t k, int, int64_t off) { memcpy(buf.data() + off, p, (size_t)k); return true; };
        auto settle = [&](int) { return true; };
        if (ring.take(100, copy, settle) != 100 || memcmp(buf.data(), data.data(), 100) != 0) { printf("the first bytes\n"); bad = 1; }
        ring.abandon();
        // what was read ahead may still be handed out; behind it the ring says it was left, never that the stream ended
        int64_t r = 1;
        for (int i = 0; !bad && i < 1 << 22 && r > 0; i++) r = ring.take(100, copy, settle);
        if (!bad && r > 0) { printf("an abandoned ring goes on\n"); bad = 1; }
        if (!bad && r == 0 && R.consumed < (int64_t)data.size()) { printf("an abandoned ring ended\n"); bad = 1; }
    }                                                        // the ring joins its thread, the reader closes: the writer gets EPIPE
    writer.join();
    if (!bad) printf("ok %lld\n", (long long)data.size());
    return bad;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: stream_core <seed> <bytes> pieces <piece> <request> | empty | closed\n"); return 2; }
    signal(SIGPIPE, SIG_IGN);
    const uint64_t seed = strtoull(argv[1], nullptr, 10);
    std::vector<uint8_t> data((size_t)atoll(argv[2]));
    std::mt19937_64 rng(seed);
    for (auto &b : data) b = (uint8_t)rng();
    const std::string mode = argv[3];
    if (mode == "pieces" && argc == 6) return pieces(data, seed, atoll(argv[4]), atoll(argv[5]));
    if (mode == "ring" && argc == 7) return ring(data, seed, atoll(argv[4]), atoll(argv[5]), atoll(argv[6]));
    if (mode == "abandon" && argc == 6) return abandon(data, seed, atoll(argv[4]), atoll(argv[5]));
    if (mode == "empty") {
        int fds[2];
        if (pipe(fds) != 0) { printf("pipe failed\n"); return 1; }
        ::close(fds[1]);
        m6a_stream::Reader R(fds[0], true, "the pipe");
        uint8_t b[8];
        const bool ok = R.at_eof() == 1 && R.fill(b, 8) == 0 && R.at_eof() == 1 && R.consumed == 0 && !R.failed;
        printf(ok ? "ok 0\n" : "an empty pipe is not at its end\n");
        return ok ? 0 : 1;
    }
    if (mode == "closed") {
        int fds[2];
        if (pipe(fds) != 0) { printf("pipe failed\n"); return 1; }
        ::close(fds[0]);
        ::close(fds[1]);
        uint8_t b[8];
        m6a_stream::Reader R(fds[0], false, "gone.txt"), Q(fds[0], false, "-");
        const bool ok = R.fill(b, 8) == -1 && R.failed && R.error == "cannot read gone.txt" && R.at_eof() == -1 && R.fill(b, 1) == -1 &&
                        Q.at_eof() == -1 && Q.error == "cannot read -" && Q.fill(b, 8) == -1;
        printf(ok ? "ok 0\n" : "a closed descriptor is not an error\n");
        return ok ? 0 : 1;
    }
    fprintf(stderr, "unknown mode\n");
    return 2;
}
