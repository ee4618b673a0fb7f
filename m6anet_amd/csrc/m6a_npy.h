// m6a_npy.h -- the host arithmetic of data.read_representation.npy as m6a_prep_sites_write_read_representation writes it
// (include/m6a.h; the writer itself is m6a_npy_write.h): the header's bytes, where a row lies in the file, and how the sites
// are cut into rounds.  Plain C++ with no HIP in it, so tests/npy_core_main.cpp runs it under the sanitizers;
// tests/repr_file_statement.py states the same in plain Python.
//
// The file is NumPy's .npy version 1.0 of a C-ordered [n_rows][32] array of '<f4' or '<f2', byte for byte what
// np.lib.format.open_memmap(path, mode="w+", dtype=np.float32 | np.float16, shape=(n_rows, 32)) leaves in front of the rows
// (numpy/lib/format.py: _write_array_header, _wrap_header; NumPy 1.24 and later):
//     "\x93NUMPY"  0x01 0x00  <u16 little-endian: the length L of what follows>
//     {'descr': '<f4', 'fortran_order': False, 'shape': (<n_rows>, 32), }
//     21 - (decimal digits of n_rows) spaces      NumPy's room for a first axis that grows: dictionary + room has one length
//     p spaces, p = 64 - ((10 + H + 1) % 64), H = the two lines above: 1 <= p <= 64, so that 10 + L is a multiple of 64
//     "\n"
// which is 128 bytes at every n_rows below 10^21; row i begins at byte 128 + i * 32 * itemsize.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "m6a_rounds.h"

namespace m6a_npy {

constexpr int kCols = 32;                    // M6A_N_REPR
constexpr int kGrowthDigits = 21;            // numpy.lib.format.GROWTH_AXIS_MAX_DIGITS
constexpr int64_t kRoundKB = 131072;         // default M6A_REPR_ROUND_KB

// dtype: 0 = M6A_REPR_F32, 1 = M6A_REPR_F16 (checked by the caller)
inline int64_t row_bytes(int dtype) { return kCols * (dtype == 1 ? 2 : 4); }

inline std::string header(int64_t n_rows, int dtype)
{
    char dict[128], digits[32];
    const int n = snprintf(dict, sizeof dict, "{'descr': '%s', 'fortran_order': False, 'shape': (%lld, %d), }", dtype == 1 ? "<f2" : "<f4",
                           (long long)n_rows, kCols);
    const int nd = snprintf(digits, sizeof digits, "%lld", (long long)n_rows);
    std::string h(dict, (size_t)n);
    if (nd < kGrowthDigits) h.append((size_t)(kGrowthDigits - nd), ' ');
    const size_t hlen = h.size() + 1;        // and the newline
    const size_t pad = 64 - ((10 + hlen) % 64);
    const size_t len = hlen + pad;
    std::string out("\x93NUMPY\x01", 7);
    out.push_back('\0');
    out.push_back((char)(len & 255));
    out.push_back((char)(len >> 8));
    out += h;
    out.append(pad, ' ');
    out.push_back('\n');
    return out;
}

// where row `row` begins in the file
inline int64_t row_offset(int64_t n_rows, int dtype, int64_t row) { return (int64_t)header(n_rows, dtype).size() + row * row_bytes(dtype); }

// Rounds of whole sites over sites [0, S) with reads off[0..S]: round k is sites [cut[k], cut[k + 1]).  A round takes as many
// sites as hold at most max(1, round_bytes / row_bytes) rows together, and at least one: a site with more rows than that is a
// round of its own.  Returns the rows of the largest round.
inline int64_t cut_rounds(const int64_t *off, int64_t S, int64_t round_bytes, int dtype, std::vector<int64_t> &cut)
{
    const int64_t per = round_bytes / row_bytes(dtype) > 1 ? round_bytes / row_bytes(dtype) : 1;
    int64_t widest = 0;
    cut.assign(1, 0);
    m6a_rounds::cut_rounds(S, per, [&](int64_t a, int64_t b) { return off[b] - off[a]; }, [&](int64_t a, int64_t b) {
        cut.push_back(b);
        if (off[b] - off[a] > widest) widest = off[b] - off[a];
    });
    return widest;
}

}  // namespace m6a_npy
