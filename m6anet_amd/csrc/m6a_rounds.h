// m6a_rounds.h -- how a list of items is cut into rounds of bounded text.  Plain C++ with no HIP in it: the device writers use it
// through m6a_prep_kit.h, and m6a_npy.h, which tests/npy_core_main.cpp runs under the sanitizers, uses it directly.
#pragma once
#include <cstdint>

namespace m6a_rounds {

// Items [0, n) in rounds of consecutive items, on_round(a, b) for each in order: round [a, b) takes as many items as
// bytes_of(a, b) <= limit allows and at least one, so an item larger than the limit is a round of its own.  bytes_of(a, b) does not
// decrease with b.
template <class BytesOf, class OnRound> inline void cut_rounds(int64_t n, int64_t limit, BytesOf bytes_of, OnRound on_round)
{
    for (int64_t a = 0; a < n;) {
        int64_t lo = a + 1, hi = n;          // the last b with bytes_of(a, b) <= limit, at least a + 1
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo + 1) / 2;
            if (bytes_of(a, mid) <= limit) lo = mid; else hi = mid - 1;
        }
        on_round(a, lo);
        a = lo;
    }
}

}  // namespace m6a_rounds
