// m6a_expect.hip -- the site probability in closed form (include/m6a.h: m6a_site_expectation, M6A_SITE_EXPECTED).
//   site_prob = (float)(1 - m1^K), mc_sigma = sqrt(max(m2^K - (m1^K)^2, 0)), m1 = mean(1 - p), m2 = mean((1 - p)^2) in float64.
// m2^K - (m1^K)^2 cancels (a unit in the last place of a power is 1e-16 / mc_sigma in the root), so the sums and the powers are
// carried as pairs hi + lo of doubles -- two-sum, Dekker's split and two-product: IEEE additions and multiplications, no fma --
// and rounded once, in the ONE order the header states: read i joins partial i % 64, reads in increasing i, then the partials
// fold 32, 16, 8, 4, 2, 1.  Both variants follow it:
//   site_expect_wave_kernel  a wavefront per site, any bags: lane j is partial j and walks reads j, j + 64, ...; six butterfly
//                            steps.  Each wavefront takes M6A_EXPECT_UNROLL sites per turn so that their loads are in flight
//                            together (a site is a latency chain: off -> read_prob -> six shuffles).
//   site_expect_lane_kernel  a lane per site, for calls whose bags all have the same n <= 32 reads (the product's 20): partial j is
//                            read j or (0, 0), partials 32..63 are (0, 0) and pair_add(x, (0, 0)) = x for every finite pair (a
//                            partial that is not finite is NaN from its first addition on, in both variants), so the step h = 32
//                            changes nothing and the lane folds 32 registers pairs 16, 8, 4, 2, 1.  No shuffle, no off[].
// Nothing here may contract into an fma or be reassociated: the error terms below are exact only as written.
#pragma clang fp contract(off)
#include "m6a_kernels.h"

#define M6A_EXPECT_UNROLL 4

struct Pair { double hi, lo; };

__device__ __forceinline__ Pair expect_quick(double s, double e)
{
    const double hi = s + e;
    return {hi, e - (hi - s)};
}
// a + b = s + e exactly (Knuth)
__device__ __forceinline__ void expect_two_sum(double a, double b, double &s, double &e)
{
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
__device__ __forceinline__ void expect_split(double a, double &h, double &l)
{
    const double c = 134217729.0 * a;                          // 2^27 + 1
    h = c - (c - a);
    l = a - h;
}
__device__ __forceinline__ Pair pair_add_double(Pair a, double b)
{
    double s, e;
    expect_two_sum(a.hi, b, s, e);
    return expect_quick(s, e + a.lo);
}
__device__ __forceinline__ Pair pair_add(Pair a, Pair b)
{
    double s, e;
    expect_two_sum(a.hi, b.hi, s, e);
    return expect_quick(s, e + (a.lo + b.lo));
}
// Dekker's two-product of the his, the cross terms rounded
__device__ __forceinline__ Pair pair_mul(Pair a, Pair b)
{
    const double p = a.hi * b.hi;
    double ah, al, bh, bl;
    expect_split(a.hi, ah, al);
    expect_split(b.hi, bh, bl);
    const double e = ((ah * bh - p) + ah * bl + al * bh) + al * bl;
    return expect_quick(p, e + (a.hi * b.lo + a.lo * b.hi));
}

// x^K, square-and-multiply from the lowest bit of K in pairs, rounded once (the header's order)
__device__ __forceinline__ double expect_pow(double x, int K)
{
    Pair r = {1.0, 0.0}, b = {x, 0.0};
    for (int e = K; e != 0;) {
        if (e & 1) r = pair_mul(r, b);
        e >>= 1;
        if (e != 0) b = pair_mul(b, b);
    }
    return r.hi;
}

// the three results of site s from its sums (n >= 1 reads, cge of them at or above the threshold)
__device__ __forceinline__ void expect_finish(const ExpectArgs &a, int64_t s, double s1, double s2, unsigned cge, int64_t n)
{
    const double dn = (double)n;
    const double q1 = expect_pow(s1 / dn, a.K), q2 = expect_pow(s2 / dn, a.K);
    a.site_prob[s] = (float)(1.0 - q1);
    a.mod_ratio[s] = (double)cge / dn;
    if (a.mc_sigma) {
        const double v = q2 - q1 * q1;
        a.mc_sigma[s] = v < 0.0 ? 0.0 : __dsqrt_rn(v);          // a negative rounding residue is 0; NaN stays NaN
    }
}

__global__ __launch_bounds__(256) void site_expect_wave_kernel(ExpectArgs a)
{
    constexpr int U = M6A_EXPECT_UNROLL;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t t0 = wave * U; t0 < a.n_sites; t0 += n_waves * U) {
        int64_t o0[U], n[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            const bool live = t0 + k < a.n_sites;
            o0[k] = live ? a.off[t0 + k] : 0;
            n[k] = live ? a.off[t0 + k + 1] - o0[k] : 0;
        }
        Pair s1[U], s2[U];
        unsigned cge[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            s1[k] = {0.0, 0.0}; s2[k] = {0.0, 0.0}; cge[k] = 0u;
            const float *p = a.read_prob + o0[k];
            int64_t i = lane;
            for (; i + 192 < n[k]; i += 256) {                  // four loads in flight, added in index order
                const float pp[4] = {p[i], p[i + 64], p[i + 128], p[i + 192]};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const double u = 1.0 - (double)pp[q];
                    s1[k] = pair_add_double(s1[k], u);
                    s2[k] = pair_add_double(s2[k], u * u);
                    cge[k] += pp[q] >= a.thr ? 1u : 0u;
                }
            }
            for (; i < n[k]; i += 64) {
                const float pv = p[i];
                const double u = 1.0 - (double)pv;
                s1[k] = pair_add_double(s1[k], u);
                s2[k] = pair_add_double(s2[k], u * u);
                cge[k] += pv >= a.thr ? 1u : 0u;
            }
        }
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) {
#pragma unroll
            for (int k = 0; k < U; k++) {
                s1[k] = pair_add(s1[k], {__shfl_xor(s1[k].hi, h, 64), __shfl_xor(s1[k].lo, h, 64)});
                s2[k] = pair_add(s2[k], {__shfl_xor(s2[k].hi, h, 64), __shfl_xor(s2[k].lo, h, 64)});
                cge[k] += __shfl_xor(cge[k], h, 64);
            }
        }
        if (lane != 0) continue;
#pragma unroll
        for (int k = 0; k < U; k++) {
            const int64_t s = t0 + k;
            if (s >= a.n_sites) continue;
            if (n[k] <= 0) {
                a.site_prob[s] = __builtin_nanf(""); a.mod_ratio[s] = __builtin_nan("");
                if (a.mc_sigma) a.mc_sigma[s] = __builtin_nan("");
                continue;
            }
            expect_finish(a, s, s1[k].hi, s2[k].hi, cge[k], n[k]);
        }
    }
}

// the fold of 32 partials, of 1 - v (SQ = false) or of its square
template <bool SQ>
__device__ __forceinline__ double expect_fold32(const float (&v)[32])
{
    Pair f[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        double x = 1.0 - (double)v[j], y = 1.0 - (double)v[j + 16];
        if (SQ) { x = x * x; y = y * y; }
        f[j] = pair_add(pair_add_double({0.0, 0.0}, x), pair_add_double({0.0, 0.0}, y));
    }
#pragma unroll
    for (int h = 8; h >= 1; h >>= 1) {
#pragma unroll
        for (int j = 0; j < h; j++) f[j] = pair_add(f[j], f[j + h]);
    }
    return f[0].hi;
}

// VEC4: a.uniform_n is a multiple of 4 and read_prob is 16-byte aligned, so a bag is whole float4s
template <bool VEC4>
__global__ __launch_bounds__(256) void site_expect_lane_kernel(ExpectArgs a)
{
    const int n = a.uniform_n;                                  // 1..32, the same for every lane: the tests on it are scalar
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < a.n_sites; s += stride) {
        const float *p = a.read_prob + s * n;
        float v[32];                                            // reads past the bag are 1.0f: 1 - 1 = +0.0 joins their partial
        if (VEC4) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                float4 t = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
                if (4 * q < n) t = reinterpret_cast<const float4 *>(p)[q];
                v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 32; i++) v[i] = i < n ? p[i] : 1.0f;
        }
        unsigned cge = 0u;
#pragma unroll
        for (int i = 0; i < 32; i++) cge += (i < n && v[i] >= a.thr) ? 1u : 0u;
        expect_finish(a, s, expect_fold32<false>(v), expect_fold32<true>(v), cge, n);
    }
}

template __global__ void site_expect_lane_kernel<false>(ExpectArgs a);
template __global__ void site_expect_lane_kernel<true>(ExpectArgs a);

// An empty kernel per translation unit: HIP maps a code object on the first launch of any kernel in it
__global__ void m6a_touch_expect() {}
