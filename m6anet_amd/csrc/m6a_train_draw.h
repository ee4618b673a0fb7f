// m6a_train_draw.h -- which `bag` reads of a site a training step sees.  Plain C++ marked for host and device: m6a_train.hip compiles it
// for gfx950 (train_draw_kernel) and for the CPU (m6a_train_sample), and tests/train_draw_main.cpp holds it to tests/train_statement.py
// as a program of its own under ASan and UBSan.
//   rule     for position i of an epoch's `order` (site s = order[i], n = off[s + 1] - off[s] reads, n >= bag) and draw j < bag:
//              u   = the high 32 bits of mix(seed + 0x9E3779B97F4A7C15 * (64 i + j + 1))     (all of it modulo 2^64)
//              r_j = j + ((u * (n - j)) >> 32)                                               (j <= r_j < n)
//            where mix is splitmix64's output function -- so u comes from output number 64 i + j + 1 of a splitmix64 generator
//            started at `seed` -- and draw j swaps entries j and r_j of a = arange(n); the sample is a[0 .. bag): a partial
//            Fisher-Yates shuffle, so the `bag` reads are distinct.  Every (i, j) has its own word of the stream: a draw depends on
//            nothing but (seed, i, n), which is what lets every bag of every step of an epoch be drawn at once.
//   bias     (u (n - j)) >> 32 takes each of its n - j values either floor or ceil(2^32 / (n - j)) times: a value's probability is
//            off by at most 2^-32 absolutely, (n - j) / 2^32 <= n / 2^32 relatively (5e-9 at 20 reads, 2e-5 at 100 000).
//   not      the reference's stream.  It draws np.random.choice(n, 20, replace=False) inside DataLoader workers
//            (m6anet/utils/data_utils.py:213-214); with its default n_processes = 25 the workers' interleaving decides which
//            site consumes which words, so that stream is not reproducible from a seed even there.
// n < 2^32.  The entries a draw moves out of the first `bag` places are kept in a list of at most `bag` (place, value) pairs.
#ifndef M6A_TRAIN_DRAW_H
#define M6A_TRAIN_DRAW_H
#include <stdint.h>

#ifndef M6A_HD
#if defined(__HIPCC__)
#define M6A_HD __host__ __device__
#else
#define M6A_HD
#endif
#endif

namespace m6a_train_draw {

constexpr int kMaxBag = 64;

M6A_HD inline uint64_t mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

M6A_HD inline uint64_t target(uint64_t seed, uint64_t i, int j, uint64_t n)
{
    const uint64_t u = mix(seed + 0x9E3779B97F4A7C15ull * (64 * i + (uint64_t)j + 1)) >> 32;
    return (uint64_t)j + ((u * (n - (uint64_t)j)) >> 32);
}

// out[0 .. bag): the sample of site-local read numbers.  1 <= bag <= kMaxBag, bag <= n < 2^32 (the caller checks).
M6A_HD inline void draw(uint64_t seed, uint64_t i, uint64_t n, int bag, int64_t *out)
{
    int64_t place[kMaxBag], value[kMaxBag];
    int m = 0;
    for (int j = 0; j < bag; j++) out[j] = j;
    for (int j = 0; j < bag; j++) {
        const int64_t r = (int64_t)target(seed, i, j, n);
        if (r < bag) {
            const int64_t t = out[j]; out[j] = out[r]; out[r] = t;
            continue;
        }
        int k = 0;
        while (k < m && place[k] != r) k++;
        if (k == m) { place[m] = r; value[m] = r; m++; }
        const int64_t t = out[j]; out[j] = value[k]; value[k] = t;
    }
}

}  // namespace m6a_train_draw
#endif
