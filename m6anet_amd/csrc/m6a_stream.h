// m6a_stream.h -- eventalign text from a pipe: the reader the stream front half (m6a_prep.hip: StreamSource) takes its bytes from.
// Plain C++ with no HIP in it; tests/stream_core_main.cpp holds it to a seeded buffer delivered through a real pipe() in pieces of
// every size, as a program of its own under ASan and UBSan.
//   fill      the caller's buffer gets exactly the bytes asked for, or what there is before the end: read() is looped over short
//             reads and EINTR, so how the writer cut its writes never shows.
//   at_eof    whether no byte follows what has been consumed.  The reader keeps one byte of lookahead for it, so the question
//             consumes nothing: a stream that ends on a request's last byte is at its end exactly then, and one more byte is not.
//   errors    a failing read() leaves `failed` set for good and the text `cannot read <path>`; fill then returns -1, at_eof -1.
// The reader owns the descriptor when it is told so (a path it opened); descriptor 0 for `-` stays the process's.
//
// Ring: the reader run ahead by a thread of its own.  The thread fills two buffers of the caller's (the pinned chunk pair) in turn,
// each to its brim or to the stream's end, and notes with the lookahead whether the buffer holds the stream's last byte; the consumer
// takes any number of bytes in order, out of the middle of a buffer if that is where the last request ended, through two calls of
// its own: copy(ptr, len, slot, offset) starts a copy out of a buffer and settle(slot) returns when every copy out of that buffer
// is complete -- only then does the buffer go back to the thread.  So the pipe is read while the consumer is busy elsewhere, by up to
// two buffers, and the consumer never waits for a read() it does not need.
//   take      up to `want` bytes; fewer only at the stream's end; -1 after a failed read, -2 when copy() said no.
//   at_eof    whether no byte follows what take() has handed out, as the reader's.  It may wait for the buffer being filled.
//   the end   the destructor asks the thread to stop and joins it; a thread inside read() leaves when that call returns.
#ifndef M6A_STREAM_H
#define M6A_STREAM_H
#include <errno.h>
#include <stdint.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>

namespace m6a_stream {

struct Reader {
    int fd = -1;
    bool own = false, failed = false, ended = false, ahead = false;
    uint8_t next = 0;                         // the lookahead byte, when `ahead`
    int64_t consumed = 0;                     // bytes handed out so far
    std::string path, error;

    Reader() = default;
    Reader(int fd_, bool own_, const char *path_) : fd(fd_), own(own_), path(path_ ? path_ : "") {}
    Reader(const Reader &) = delete;
    Reader &operator=(const Reader &) = delete;
    ~Reader() { if (own && fd >= 0) ::close(fd); }

    // one read() that is not interrupted: > 0 bytes, 0 at the end, -1 (and `failed`) on an error
    int64_t read_some(uint8_t *dst, int64_t want)
    {
        if (failed) return -1;
        if (ended || want <= 0) return 0;
        for (;;) {
            const ssize_t r = ::read(fd, dst, (size_t)want);
            if (r < 0 && errno == EINTR) continue;
            if (r < 0) { failed = true; error = "cannot read " + path; return -1; }
            if (r == 0) ended = true;
            return (int64_t)r;
        }
    }

    // dst[0, want) from the stream; returns how many bytes arrived (fewer than `want` only at the end -- or once *stop is set,
    // which is looked at between two reads), or -1
    int64_t fill(uint8_t *dst, int64_t want, const std::atomic<bool> *stop = nullptr)
    {
        if (failed) return -1;
        int64_t got = 0;
        if (want > 0 && ahead) { dst[got++] = next; ahead = false; }
        while (got < want) {
            if (stop && stop->load()) break;
            const int64_t r = read_some(dst + got, want - got);
            if (r < 0) return -1;
            if (r == 0) break;
            got += r;
        }
        consumed += got;
        return got;
    }

    // 1: no byte follows; 0: one does (it stays unconsumed); -1: the read failed
    int at_eof()
    {
        if (failed) return -1;
        if (ahead) return 0;
        const int64_t r = read_some(&next, 1);
        if (r < 0) return -1;
        ahead = r == 1;
        return ahead ? 0 : 1;
    }
};

struct Ring {
    struct Slot { int64_t len = 0, at = 0; bool full = false, last = false; };
    Reader &R;
    uint8_t *buf[2];
    int64_t cap;
    Slot slot[2];
    int head = 0;                             // the consumer's buffer
    bool failed = false, ended = false;       // the thread gave up (a failed read, or stopped); the consumer has taken the last byte
    std::atomic<bool> stop{false};
    std::mutex mu;
    std::condition_variable cv;
    std::thread t;

    Ring(Reader &r, uint8_t *b0, uint8_t *b1, int64_t cap_) : R(r), buf{b0, b1}, cap(cap_) {}
    Ring(const Ring &) = delete;
    Ring &operator=(const Ring &) = delete;
    ~Ring()
    {
        abandon();
        if (t.joinable()) t.join();
    }

    // nothing more will be taken: the thread leaves at its next look, and a consumer waiting in take() or at_eof() gets -1
    void abandon()
    {
        stop.store(true);
        { std::lock_guard<std::mutex> lk(mu); }
        cv.notify_all();
    }

    void start() { t = std::thread([this]() { run(); }); }

    void run()
    {
        for (int tail = 0;; tail ^= 1) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&]() { return !slot[tail].full || stop.load(); });
                if (stop.load()) { failed = true; lk.unlock(); cv.notify_all(); return; }
            }
            const int64_t n = R.fill(buf[tail], cap, &stop);
            // a short buffer is the stream's last; a full one is when the lookahead finds nothing behind it
            const int e = n < 0 || stop.load() ? -1 : n < cap ? 1 : R.at_eof();
            {
                std::lock_guard<std::mutex> lk(mu);
                if (e < 0) failed = true;
                else { slot[tail].len = n; slot[tail].at = 0; slot[tail].last = e == 1; slot[tail].full = true; }
            }
            cv.notify_all();
            if (e != 0) return;
        }
    }

    // the buffer at `head`, filled: false when the thread gave up before it filled it
    bool wait_head()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&]() { return slot[head].full || failed; });
        return slot[head].full;
    }

    template <class Copy, class Settle> int64_t take(int64_t want, Copy copy, Settle settle)
    {
        int64_t got = 0;
        while (got < want && !ended) {
            if (!wait_head()) return -1;
            Slot &s = slot[head];                           // the consumer's until it hands the buffer back
            const int64_t k = std::min(want - got, s.len - s.at);
            if (k > 0 && !copy((const uint8_t *)buf[head] + s.at, k, head, got)) return -2;
            got += k;
            s.at += k;
            if (s.at < s.len) continue;
            if (!settle(head)) return -2;
            if (s.last) { ended = true; break; }
            {
                std::lock_guard<std::mutex> lk(mu);
                s.full = false;
                head ^= 1;
            }
            cv.notify_all();
        }
        return got;
    }

    int at_eof()
    {
        if (ended) return 1;
        if (!wait_head()) return -1;
        if (slot[head].at < slot[head].len) return 0;
        ended = true;                                       // an empty buffer: the stream held nothing at all
        return 1;
    }
};

}  // namespace m6a_stream
#endif
