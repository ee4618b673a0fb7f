// m6a_pairs.h -- the scheme of every test on pairs of sites, one site from each of two sets (m6a_ranksum.hip, m6a_ks.hip), stated once:
// a wavefront per pair, the pooled sample a ++ b walked in chunks of 64, both bags streamed through the wavefront's LDS tile and read
// back as float4 broadcasts.  What a lane counts, and how a pair closes, is the unit's own.  Here are
//   PairsIn        the input block of every pair kernel; a kernel's argument struct is this block, its own outputs and err behind them,
//                  where the kernels had it (the order of the kernel arguments decides the scalar registers of the whole build)
//   pair_bags      pair index -> sites -> offsets, every one checked before anything is read through it
//   pair_fill, pair_fill_rows   a tile of values, or of rows [cnt][9] turned column-major, into LDS
//   pair_wave, pair_first, pair_step, pair_launch   the grid-stride walk of the wavefronts and the grid rule
//   pair_call      the entry point on host or device pointers (the convention of m6a_ctx.h), the four outputs staged type-blind
#ifndef M6A_PAIRS_H
#define M6A_PAIRS_H
#include "m6a_ctx.h"
#include "m6a_ranksum.h"

#define M6A_PAIR_TILE 256                                     // values (or rows) per wavefront in LDS: 1 KB, 4 KB per block -- occupancy stays with the registers
#define M6A_PAIR_COLS M6A_N_FEATURES
#define M6A_PAIR_STRIDE (M6A_PAIR_TILE + 4)                   // floats from a column of rows to the next: whole float4s, and 4 c + r (mod 32)
                                                              // is the bank of a transposing write, not r alone -- 9.1 KB per wavefront
#define M6A_PAIR_WAVES 4                                      // wavefronts, so pairs, per block of 256

namespace m6a_detail {

struct PairsIn {
    const float *v_a, *v_b;           // [off_a[n_sites_a]], [off_b[n_sites_b]] values, or rows of nine (the signal calls)
    const int64_t *off_a, *off_b;     // [n_sites + 1]
    const int64_t *pair_a, *pair_b;   // [n_pairs] or null: the identity
    int64_t n_sites_a, n_sites_b, n_pairs;
};

// the pair's two bags as rows [a0, a1) and [b0, b1), or bad: nothing is read through an index or an offset before it is checked
__device__ __forceinline__ bool pair_bags(const PairsIn &a, int64_t k, int64_t &a0, int64_t &a1, int64_t &b0, int64_t &b1)
{
    const int64_t ia = a.pair_a ? a.pair_a[k] : k, ib = a.pair_b ? a.pair_b[k] : k;
    a0 = a1 = b0 = b1 = 0;
    if (ia < 0 || ia >= a.n_sites_a || ib < 0 || ib >= a.n_sites_b) return false;
    a0 = a.off_a[ia]; a1 = a.off_a[ia + 1];
    b0 = a.off_b[ib]; b1 = a.off_b[ib + 1];
    return !(a0 < 0 || a1 < a0 || a1 > a.off_a[a.n_sites_a] || b0 < 0 || b1 < b0 || b1 > a.off_b[a.n_sites_b]);
}

// cnt <= M6A_PAIR_TILE floats from p into the tile, NaN (which compares false) up to the next multiple of 4; ordered against the
// reads around it
__device__ __forceinline__ void pair_fill(float *tile, const float *p, int cnt, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < M6A_PAIR_TILE / 64; k++) {
        if (k * 64 >= cnt) break;                               // uniform
        const int j = k * 64 + lane;
        tile[j] = j < cnt ? p[j] : __builtin_nanf("");
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// cnt <= M6A_PAIR_TILE rows [cnt][9] from `rows` into the tile, column c at tile + c * M6A_PAIR_STRIDE, every column padded with NaN
// to the next multiple of 4; 9 cnt contiguous dwords, lane l taking dword f0 + l (a row is 36 bytes, so no wider load has an alignment
// to rely on).  Ordered against the reads around it as pair_fill is
__device__ __forceinline__ void pair_fill_rows(float *tile, const float *rows, int cnt, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int n_f = cnt * M6A_PAIR_COLS;
#pragma unroll 4
    for (int f0 = 0; f0 < n_f; f0 += 64) {                      // uniform
        const int f = f0 + lane;
        if (f < n_f) {
            const int r = f / M6A_PAIR_COLS, c = f - r * M6A_PAIR_COLS;
            tile[c * M6A_PAIR_STRIDE + r] = rows[f];
        }
    }
    const int pad = (4 - (cnt & 3)) & 3;                        // rows cnt .. cnt + pad - 1 of every column: at most 3, below the stride
    if (lane < 3 * M6A_PAIR_COLS) {
        const int c = lane / 3, d = lane - 3 * c;
        if (d < pad) tile[c * M6A_PAIR_STRIDE + cnt + d] = __builtin_nanf("");
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned pair_one(bool hit) { return hit ? 1u : 0u; }

// the walk: wavefront w of a block owns lds[w] and the pairs pair_first(w), + pair_step(), ... below n_pairs (a kernel reads the step
// once, before its loop)
__device__ __forceinline__ int pair_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ int64_t pair_first(int w) { return (int64_t)blockIdx.x * M6A_PAIR_WAVES + w; }
__device__ __forceinline__ int64_t pair_step() { return (int64_t)gridDim.x * M6A_PAIR_WAVES; }

// the launch on the context's stream: a pair per wavefront, four per block, n_cu * 64 blocks at most -- more blocks than are resident,
// so that ragged bags balance over the order in which blocks are handed out
template <class Args>
int pair_launch(m6a_ctx *c, void (*kernel)(Args), const Args &a)
{
    const unsigned blocks = (unsigned)std::min<int64_t>((a.n_pairs + M6A_PAIR_WAVES - 1) / M6A_PAIR_WAVES, (int64_t)c->n_cu * 64);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * M6A_PAIR_WAVES), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    return M6A_OK;
}

// An entry point: a bag's element is `cols` float32 (1: a value, 9: a row of X) and a pair's output `cols` values in each of the four
// arrays of `out`, all 8 bytes wide, so they are staged without their types; out[i] may be NULL unless required[i].
// launch(in, out) queues the kernel on device arrays.  The calls are synchronous on host pointers and one at a time, so all of them
// stage in c->sRank: [0] v_a [1] off_a [2] v_b [3] off_b [4] pair_a [5] pair_b in, [6..9] out[0..3]
template <class Launch>
int pair_call(m6a_ctx *c, int cols, const float *v_a, const int64_t *off_a, int64_t n_sites_a, const float *v_b, const int64_t *off_b,
              int64_t n_sites_b, const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs, void *const (&out)[4],
              const bool (&required)[4], const char *sentence, Launch launch)
{
    HintScope hint_scope(c);
    int rc = enter(c);
    if (rc) return rc;
    if (n_sites_a < 0 || n_sites_b < 0 || n_pairs < 0) return fail(c, M6A_EINVAL, "n_sites_a, n_sites_b and n_pairs must be >= 0");
    if (n_pairs == 0) return M6A_OK;
    if ((!pair_a || !pair_b) && (n_pairs != n_sites_a || n_pairs != n_sites_b))
        return fail(c, M6A_EINVAL, "a NULL pair array is the identity and needs n_pairs == n_sites_a == n_sites_b");
    bool missing = !v_a || !off_a || !v_b || !off_b;
    for (int i = 0; i < 4; i++) missing = missing || (required[i] && !out[i]);
    if (missing) return fail(c, M6A_EINVAL, "null pointer argument");
    HIPCHK(c, hipSetDevice(c->device));
    const int dev = same_side(c, v_a, {off_a, v_b, off_b, pair_a, pair_b, out[0], out[1], out[2], out[3]}, sentence);
    if (dev < 0) return dev;
    PairsIn in{v_a, v_b, off_a, off_b, pair_a, pair_b, n_sites_a, n_sites_b, n_pairs};
    if (dev) return launch(in, out);
    rc = csr_check(c, off_a, n_sites_a);
    if (rc) return rc;
    rc = csr_check(c, off_b, n_sites_b);
    if (rc) return rc;
    for (int64_t k = 0; k < n_pairs; k++) {
        if (pair_a && (pair_a[k] < 0 || pair_a[k] >= n_sites_a)) return fail(c, M6A_EINVAL, "pair_a[%lld] = %lld is outside the %lld sites of the first set", (long long)k, (long long)pair_a[k], (long long)n_sites_a);
        if (pair_b && (pair_b[k] < 0 || pair_b[k] >= n_sites_b)) return fail(c, M6A_EINVAL, "pair_b[%lld] = %lld is outside the %lld sites of the second set", (long long)k, (long long)pair_b[k], (long long)n_sites_b);
    }
    DevBuf *s = c->sRank;
    const size_t pb = (size_t)n_pairs * 8, ob = pb * (size_t)cols, el = (size_t)cols * sizeof(float);
    HIPCHK(c, stage_in(c, s[0], v_a, (size_t)off_a[n_sites_a] * el));
    HIPCHK(c, stage_in(c, s[1], off_a, (size_t)(n_sites_a + 1) * 8));
    HIPCHK(c, stage_in(c, s[2], v_b, (size_t)off_b[n_sites_b] * el));
    HIPCHK(c, stage_in(c, s[3], off_b, (size_t)(n_sites_b + 1) * 8));
    if (pair_a) HIPCHK(c, stage_in(c, s[4], pair_a, pb));
    if (pair_b) HIPCHK(c, stage_in(c, s[5], pair_b, pb));
    for (int i = 6; i < 10; i++) HIPCHK(c, s[i].ensure(ob));
    in.v_a = (const float *)s[0].p; in.off_a = (const int64_t *)s[1].p; in.v_b = (const float *)s[2].p; in.off_b = (const int64_t *)s[3].p;
    in.pair_a = pair_a ? (const int64_t *)s[4].p : nullptr; in.pair_b = pair_b ? (const int64_t *)s[5].p : nullptr;
    void *const staged[4] = {out[0] ? s[6].p : nullptr, out[1] ? s[7].p : nullptr, out[2] ? s[8].p : nullptr, out[3] ? s[9].p : nullptr};
    rc = launch(in, staged);
    if (rc) return rc;
    for (int i = 0; i < 4; i++) if (out[i]) HIPCHK(c, stage_out(c, out[i], s[6 + i], ob));
    return sync_and_check(c);
}

}  // namespace m6a_detail

#endif
