// m6a_train.hip -- training of the m6anet.toml model: training-mode forward, backward and Adam (include/m6a.h: m6a_train_*; the
// operation is stated once in tests/train_statement.py).  Internal declarations: m6a_ctx.h.
//
// One step is a chain of six plain launches on the context's stream (seven with gradient clipping on, where train_adam_kernel is
// train_grad_kernel -- the same folds, the gradient and a sum of g^2 per block -- and train_clip_adam_kernel -- the norm, the scale,
// Adam: every block needs the whole gradient's norm, and that takes a kernel boundary); nothing comes back to the host between steps:
//   train_fwd1_kernel    per chunk of reads: gather x (features | three embeddings), z1 = W1 x + b1, and the chunk's sums of z1 and
//                        z1^2 per hidden unit in float64;
//   train_stats_kernel   the chunks' sums in chunk order -> mu, 1 / sqrt(var + eps); the running statistics;
//   train_fwd2_kernel    a lane per read, a wave on whole bags: batch norm, ReLU, layer 2, the head, the bag's product with its
//                        prefix and suffix products, the loss term, dL/dlogit, dL/dh2, dL/dy1 and the wave's sums for dgamma, dbeta;
//   train_fold_kernel    the waves' sums in wave order -> dgamma, dbeta; the loss;
//   train_bwd1_kernel    per chunk of reads, a thread per hidden unit: batch norm backward, and the chunk's part of dW1, db1, dW2,
//                        db2, dW3, db3; dL/dx of the six embedding inputs per read;
//   train_adam_kernel    the chunks' parts in chunk order (the embedding: a wave per entry over the bags that carry the k-mer),
//                        the gradient, Adam.
// The same step cut at s for a caller with its own loss and optimizer (m6a_train_forward / m6a_train_backward): the forward half is
// train_fwd1_kernel, train_stats_kernel and train_fwd2_kernel<kForward>; the backward half train_fwd2_kernel<kBackward> (dL/ds read
// from memory), train_fold_kernel, train_bwd1_kernel and train_grad_kernel, on the activations the forward left in the scratch.
// Sums run in a fixed order and there is no atomic on a float anywhere: the same state and batch give the same bits.
#include "m6a_ctx.h"
#include "m6a_train_draw.h"

using namespace m6a_detail;

namespace {

constexpr int kH1 = 150, kIn = 15, kH2 = 32, kTile = 32, kMaxChunks = 256, kXs = 16;
constexpr int oE = 0, oW1 = 132, oB1 = 2382, oGamma = 2532, oBeta = 2682, oMean = 2832, oVar = 2982, oW2 = 3132, oB2 = 7932, oW3 = 7964,
              oB3 = 7996;
constexpr int kRow = 10;            // 150 = 15 * kRow
constexpr int kBatch = 8;           // independent loads issued together in the folds
constexpr int64_t kMaxBatchReads = (int64_t)1 << 20;
constexpr double kBnEps = 1e-5, kMomentum = 0.1;

enum { kErrReads = 1, kErrKmer = 2, kErrLabel = 3, kErrOrder = 4 };

__device__ inline void report(unsigned long long *err, int64_t index, int kind)
{
    atomicMin(err, ((unsigned long long)index << 3) | (unsigned)kind);
}

// every site of a call: >= bag reads (off != null), k-mer ids 0..65, label 0 or 1
__global__ void train_check_sites_kernel(const uint8_t *km, const int64_t *off, const float *y, int64_t S, int bag, unsigned long long *err)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (off) {
        const int64_t n = off[s + 1] - off[s];
        if (n < bag || n > 0xffffffffll) report(err, s, kErrReads);
    }
    if (km[s * 3] >= M6A_N_KMERS || km[s * 3 + 1] >= M6A_N_KMERS || km[s * 3 + 2] >= M6A_N_KMERS) report(err, s, kErrKmer);
    const float v = y[s];
    if (!(v == 0.f || v == 1.f)) report(err, s, kErrLabel);
}

// m6a_train_forward has no labels to check: the k-mer ids alone
__global__ void train_check_kmers_kernel(const uint8_t *km, int64_t S, unsigned long long *err)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (km[s * 3] >= M6A_N_KMERS || km[s * 3 + 1] >= M6A_N_KMERS || km[s * 3 + 2] >= M6A_N_KMERS) report(err, s, kErrKmer);
}

// every position of an epoch's order: the site exists; its `bag` reads (m6a_train_draw.h) as global read indices
__global__ void train_draw_kernel(const int64_t *off, const int64_t *order, int64_t n_order, int64_t S, int bag, uint64_t seed,
                                  int64_t *ridx, unsigned long long *err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_order) return;
    const int64_t s = order[i];
    int64_t out[m6a_train_draw::kMaxBag];
    int64_t lo = 0;
    bool ok = s >= 0 && s < S;
    if (!ok) report(err, i, kErrOrder);
    if (ok) {
        lo = off[s];
        const int64_t n = off[s + 1] - lo;
        ok = n >= bag && n <= 0xffffffffll;                     // reported by train_check_sites_kernel
        if (ok) m6a_train_draw::draw(seed, (uint64_t)i, (uint64_t)n, bag, out);
    }
    for (int j = 0; j < bag; j++) ridx[i * bag + j] = ok ? lo + out[j] : 0;
}

struct Batch {
    const float *X;             // [R][9]
    const int64_t *ridx;        // [N] read of X behind each read of the batch, or null: the batch is X[0 .. N)
    const uint8_t *km;          // [S][3]
    const int64_t *sidx;        // [B] site of each bag, or null: bag b is site b
    const float *y;             // [S]
    int64_t B, N;
    int bag;
};

__global__ __launch_bounds__(192) void train_fwd1_kernel(Batch bt, int64_t chunk_reads, const float *__restrict__ P, float *__restrict__ xbuf,
                                                         float *__restrict__ z1, double *__restrict__ part)
{
    __shared__ float xs[kTile][kXs];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * chunk_reads, c1 = min(bt.N, c0 + chunk_reads);
    float w[kIn], b = 0.f;
    if (tid < kH1) {
        for (int k = 0; k < kIn; k++) w[k] = P[oW1 + tid * kIn + k];
        b = P[oB1 + tid];
    }
    double s = 0.0, ss = 0.0;
    for (int64_t t0 = c0; t0 < c1; t0 += kTile) {
        const int nt = (int)min((int64_t)kTile, c1 - t0);
        for (int e = tid; e < nt * kIn; e += 192) {
            const int r = e / kIn, k = e - r * kIn;
            const int64_t n = t0 + r;
            float v;
            if (k < M6A_N_FEATURES) {
                v = bt.X[(bt.ridx ? bt.ridx[n] : n) * M6A_N_FEATURES + k];
            } else {
                const int64_t bg = n / bt.bag, site = bt.sidx ? bt.sidx[bg] : bg;
                v = P[oE + (int)bt.km[site * 3 + ((k - M6A_N_FEATURES) >> 1)] * 2 + ((k - M6A_N_FEATURES) & 1)];
            }
            xs[r][k] = v;
            xbuf[n * kXs + k] = v;
        }
        __syncthreads();
        if (tid < kH1)
            for (int r = 0; r < nt; r++) {
                float z = b;
                for (int k = 0; k < kIn; k++) z = fmaf(w[k], xs[r][k], z);
                z1[(t0 + r) * kH1 + tid] = z;
                s += (double)z;
                ss += (double)z * (double)z;
            }
        __syncthreads();
    }
    if (tid < kH1) {
        part[(size_t)blockIdx.x * 2 * kH1 + tid] = s;
        part[(size_t)blockIdx.x * 2 * kH1 + kH1 + tid] = ss;
    }
}

// stat[0 .. 150) = mu, stat[150 .. 300) = 1 / sqrt(var + eps)
__global__ void train_stats_kernel(const double *__restrict__ part, int n_chunks, int64_t N, float *__restrict__ P, double *__restrict__ stat)
{
    const int j = threadIdx.x;
    if (j >= kH1) return;
    double s = 0.0, ss = 0.0;
    for (int c0 = 0; c0 < n_chunks; c0 += kBatch) {                // kBatch loads in flight, the additions in chunk order
        double a[kBatch], b[kBatch];
        for (int u = 0; u < kBatch; u++) {
            const bool in = c0 + u < n_chunks;
            a[u] = in ? part[(size_t)(c0 + u) * 2 * kH1 + j] : 0.0;
            b[u] = in ? part[(size_t)(c0 + u) * 2 * kH1 + kH1 + j] : 0.0;
        }
        for (int u = 0; u < kBatch; u++) if (c0 + u < n_chunks) { s += a[u]; ss += b[u]; }
    }
    const double mu = s / (double)N, var = fmax(ss / (double)N - mu * mu, 0.0);
    stat[j] = mu;
    stat[kH1 + j] = 1.0 / sqrt(var + kBnEps);
    P[oMean + j] = (float)((1.0 - kMomentum) * (double)P[oMean + j] + kMomentum * mu);
    P[oVar + j] = (float)((1.0 - kMomentum) * (double)P[oVar + j] + kMomentum * (var * (double)N / (double)(N - 1)));
}

__device__ inline double wave_sum(double v)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// train_fwd2_kernel is one body behind three kernels, the two halves m6a_train_forward / m6a_train_backward cut a step into among
// them; the mode is a compile-time constant, so each instantiation holds its own half only:
//   kFused     the step's kernel: everything below, dL/ds from BCELoss and the labels bt.y;
//   kForward   up to s: h2buf and y_pred are written, nothing else (dlogit, dy1, wpart, loss_term may be null);
//   kBackward  from the kept h2buf: the head and p again (the same operations on the same values: the forward's bits), the products,
//              then dL/ds READ from bt.y [B] -- the place of the labels holds the upstream gradient -- and everything behind it.
//              h2buf is only read; loss_term and y_pred may be null.
// bags_per_wave = 64 / bag whole bags per wave, lane = read.  wpart [n_waves][300]: the wave's sums of dy1 (dbeta) and dy1 xhat (dgamma).
enum { kFused = 0, kForward = 1, kBackward = 2 };

template <int Mode>
__global__ __launch_bounds__(256) void train_fwd2_kernel(Batch bt, int bags_per_wave, int64_t n_waves, float inv_B, const float *__restrict__ z1,
                                                         const double *__restrict__ stat, const float *__restrict__ P, float *__restrict__ h2buf,
                                                         float *__restrict__ dlogit, float *__restrict__ dy1, float *__restrict__ wpart,
                                                         float *__restrict__ loss_term, float *__restrict__ y_pred)
{
    __shared__ float w2t[kH1 * kH2];            // [j][i]
    __shared__ double mus[kH1], iss[kH1];
    __shared__ float gs[kH1], bs[kH1];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int e = tid; e < kH1 * kH2; e += 256) { const int i = e / kH1, j = e - i * kH1; w2t[j * kH2 + i] = P[oW2 + e]; }
    for (int j = tid; j < kH1; j += 256) { mus[j] = stat[j]; iss[j] = stat[kH1 + j]; gs[j] = P[oGamma + j]; bs[j] = P[oBeta + j]; }
    __syncthreads();
    const int64_t wave = (int64_t)blockIdx.x * 4 + (tid >> 6);
    if (wave >= n_waves) return;                // no barrier below
    const int64_t bag0 = wave * bags_per_wave;
    const int nb = (int)min((int64_t)bags_per_wave, bt.B - bag0), bag = bt.bag;
    const bool active = lane < nb * bag;
    const int lb = active ? lane / bag : 0, pos = active ? lane - lb * bag : 0;
    const int64_t b = bag0 + lb, n = b * bag + pos;

    float acc[kH2];
    for (int i = 0; i < kH2; i++) acc[i] = P[oB2 + i];
    float p = 0.f;
    if (active) {
        if constexpr (Mode == kBackward) {
            for (int i = 0; i < kH2; i++) acc[i] = h2buf[n * kH2 + i];
        } else {
            for (int j0 = 0; j0 < kH1; j0 += kRow) {             // kRow values of the read's row of z1 loaded together
                float z[kRow];
                for (int u = 0; u < kRow; u++) z[u] = z1[n * kH1 + j0 + u];
                for (int u = 0; u < kRow; u++) {
                    const int j = j0 + u;
                    const float xh = (float)(((double)z[u] - mus[j]) * iss[j]);
                    const float a = fmaxf(fmaf(gs[j], xh, bs[j]), 0.f);
                    for (int i = 0; i < kH2; i++) acc[i] = fmaf(w2t[j * kH2 + i], a, acc[i]);
                }
            }
        }
        float logit = P[oB3];
        for (int i = 0; i < kH2; i++) {
            if constexpr (Mode != kBackward) h2buf[n * kH2 + i] = acc[i];
            logit = fmaf(P[oW3 + i], fmaxf(acc[i], 0.f), logit);
        }
        p = 1.0f / (1.0f + expf(-logit));
    }
    // the bag's product, left to right, with the products before and behind this read
    const float q = active ? 1.0f - p : 1.0f;
    const int base = lb * bag;
    float prod = 1.0f, pre = 1.0f, suf = 1.0f;
    for (int k = 0; k < bag; k++) {
        const float qk = __shfl(q, (base + k) & 63);
        if (k == pos) pre = prod;
        prod *= qk;
    }
    for (int k = bag - 1; k >= 0; k--) {
        const float qk = __shfl(q, (base + k) & 63);
        if (k > pos) suf *= qk;
    }
    if constexpr (Mode == kForward) {
        if (active && pos == 0) y_pred[b] = 1.0f - prod;
        return;
    }
    float dl = 0.f;
    if (active) {
        if constexpr (Mode == kBackward) {
            dl = bt.y[b] * (pre * suf) * ((1.0f - p) * p);
            dlogit[n] = dl;
        } else {
            const float s = 1.0f - prod;
            const float yb = bt.y[bt.sidx ? bt.sidx[b] : b];
            const float dLds = (s - yb) / fmaxf((1.0f - s) * s, 1e-12f) * inv_B;
            dl = dLds * (pre * suf) * ((1.0f - p) * p);
            dlogit[n] = dl;
            if (pos == 0) {
                const float ls = fmaxf(logf(s), -100.0f), l1s = fmaxf(logf(1.0f - s), -100.0f);
                loss_term[b] = -(yb * ls + (1.0f - yb) * l1s);
                y_pred[b] = s;
            }
        }
    }
    for (int i = 0; i < kH2; i++) acc[i] = acc[i] > 0.f ? dl * P[oW3 + i] : 0.f;          // dL/dh2
    for (int j0 = 0; j0 < kH1; j0 += kRow) {
        float z[kRow];
        for (int u = 0; u < kRow; u++) z[u] = active ? z1[n * kH1 + j0 + u] : 0.f;
        float d[kRow], dx[kRow];
        for (int u = 0; u < kRow; u++) {
            const int j = j0 + u;
            d[u] = dx[u] = 0.f;
            if (active) {
                const float xh = (float)(((double)z[u] - mus[j]) * iss[j]);
                const float y1 = fmaf(gs[j], xh, bs[j]);
                float da = 0.f;
                for (int i = 0; i < kH2; i++) da = fmaf(w2t[j * kH2 + i], acc[i], da);
                d[u] = y1 > 0.f ? da : 0.f;
                dx[u] = d[u] * xh;
                dy1[n * kH1 + j] = d[u];
            }
        }
        // the 2 kRow wave sums side by side, each the butterfly of wave_sum: their exchanges overlap instead of waiting for each other
        for (int m = 32; m >= 1; m >>= 1)
            for (int u = 0; u < kRow; u++) { d[u] += __shfl_xor(d[u], m); dx[u] += __shfl_xor(dx[u], m); }
        if (lane == 0)
            for (int u = 0; u < kRow; u++) { wpart[wave * 2 * kH1 + j0 + u] = d[u]; wpart[wave * 2 * kH1 + kH1 + j0 + u] = dx[u]; }
    }
}

// tot[0 .. 150) = dbeta, tot[150 .. 300) = dgamma; *loss = mean of the B loss terms
__global__ __launch_bounds__(256) void train_fold_kernel(const float *__restrict__ wpart, int64_t n_waves, double *__restrict__ tot,
                                                         const float *__restrict__ loss_term, int64_t B, float *__restrict__ loss)
{
    const int tid = threadIdx.x;
    if (tid < kH1) {
        double sb = 0.0, sg = 0.0;
        for (int64_t w0 = 0; w0 < n_waves; w0 += kBatch) {
            float a[kBatch], b[kBatch];
            for (int u = 0; u < kBatch; u++) {
                const bool in = w0 + u < n_waves;
                a[u] = in ? wpart[(w0 + u) * 2 * kH1 + tid] : 0.f;
                b[u] = in ? wpart[(w0 + u) * 2 * kH1 + kH1 + tid] : 0.f;
            }
            for (int u = 0; u < kBatch; u++) if (w0 + u < n_waves) { sb += (double)a[u]; sg += (double)b[u]; }
        }
        tot[tid] = sb;
        tot[kH1 + tid] = sg;
    } else if (tid >= 192) {                    // one whole wave
        const int lane = tid - 192;
        double a = 0.0;
        for (int64_t b = lane; b < B; b += 64) a += (double)loss_term[b];
        a = wave_sum(a);
        if (lane == 0) *loss = (float)(a / (double)B);
    }
}

// part [n_chunks][M6A_N_WEIGHTS] in blob order: the chunk's share of dW1, db1, dW2, db2, dW3, db3.  dxe [N][6].
__global__ __launch_bounds__(192) void train_bwd1_kernel(int64_t N, int64_t chunk_reads, const float *__restrict__ z1, const float *__restrict__ dy1,
                                                         const float *__restrict__ xbuf, const float *__restrict__ h2buf,
                                                         const float *__restrict__ dlogit, const double *__restrict__ stat,
                                                         const double *__restrict__ tot, const float *__restrict__ P, float *__restrict__ part,
                                                         float *__restrict__ dxe)
{
    __shared__ float xs[kTile][kXs], dhs[kTile][kH2], g3s[kTile][kH2], dls[kTile], dzs[kTile][kH1], w1e[kH1][6], w3s[kH2];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * chunk_reads, c1 = min(N, c0 + chunk_reads);
    for (int e = tid; e < kH1 * 6; e += 192) { const int j = e / 6, k = e - j * 6; w1e[j][k] = P[oW1 + j * kIn + M6A_N_FEATURES + k]; }
    if (tid < kH2) w3s[tid] = P[oW3 + tid];
    float aW1[kIn], aW2[kH2], ab1 = 0.f, a2 = 0.f, a3 = 0.f;       // tid >= 150: a2, a3 = db2 | dW3 of unit tid - 150, db3 in thread 182
    for (int k = 0; k < kIn; k++) aW1[k] = 0.f;
    for (int i = 0; i < kH2; i++) aW2[i] = 0.f;
    double mu = 0.0, istd = 0.0;
    float g = 0.f, bta = 0.f, cg = 0.f, mb = 0.f, mg = 0.f;
    if (tid < kH1) {
        mu = stat[tid]; istd = stat[kH1 + tid];
        g = P[oGamma + tid]; bta = P[oBeta + tid];
        cg = (float)((double)g * istd);
        mb = (float)(tot[tid] / (double)N);
        mg = (float)(tot[kH1 + tid] / (double)N);
    }
    __syncthreads();
    for (int64_t t0 = c0; t0 < c1; t0 += kTile) {
        const int nt = (int)min((int64_t)kTile, c1 - t0);
        for (int e = tid; e < nt * kIn; e += 192) { const int r = e / kIn, k = e - r * kIn; xs[r][k] = xbuf[(t0 + r) * kXs + k]; }
        for (int e = tid; e < nt * kH2; e += 192) {
            const int r = e >> 5, i = e & 31;
            const float h = h2buf[(t0 + r) * kH2 + i], dl = dlogit[t0 + r];
            dhs[r][i] = h > 0.f ? dl * w3s[i] : 0.f;
            g3s[r][i] = dl * fmaxf(h, 0.f);
            if (i == 0) dls[r] = dl;
        }
        __syncthreads();
        if (tid < kH1) {
            for (int r = 0; r < nt; r++) {
                const int64_t n = t0 + r;
                const float xh = (float)(((double)z1[n * kH1 + tid] - mu) * istd);
                const float a1 = fmaxf(fmaf(g, xh, bta), 0.f);
                const float dz = cg * ((dy1[n * kH1 + tid] - mb) - xh * mg);
                dzs[r][tid] = dz;
                ab1 += dz;
                for (int k = 0; k < kIn; k++) aW1[k] = fmaf(dz, xs[r][k], aW1[k]);
                for (int i = 0; i < kH2; i++) aW2[i] = fmaf(dhs[r][i], a1, aW2[i]);
            }
        } else if (tid < kH1 + kH2) {
            for (int r = 0; r < nt; r++) { a2 += dhs[r][tid - kH1]; a3 += g3s[r][tid - kH1]; }
        } else if (tid == kH1 + kH2) {
            for (int r = 0; r < nt; r++) a3 += dls[r];
        }
        __syncthreads();
        if (tid < nt * 6) {                     // kTile * 6 = 192 = the block
            const int r = tid / 6, k = tid - r * 6;
            float a = 0.f;
            for (int j = 0; j < kH1; j++) a = fmaf(w1e[j][k], dzs[r][j], a);
            dxe[(t0 + r) * 6 + k] = a;
        }
        __syncthreads();
    }
    float *out = part + (size_t)blockIdx.x * M6A_N_WEIGHTS;
    if (tid < kH1) {
        for (int k = 0; k < kIn; k++) out[oW1 + tid * kIn + k] = aW1[k];
        out[oB1 + tid] = ab1;
        for (int i = 0; i < kH2; i++) out[oW2 + i * kH1 + tid] = aW2[i];
    } else if (tid < kH1 + kH2) {
        out[oB2 + tid - kH1] = a2;
        out[oW3 + tid - kH1] = a3;
    } else if (tid == kH1 + kH2) {
        out[oB3] = a3;
    }
}

struct AdamArgs { float step_size, bc2_sqrt, beta1, beta2, one_minus_beta1, one_minus_beta2, eps, weight_decay; };

__device__ inline void adam_apply(int e, float gr, const AdamArgs &a, float *P, float *M, float *V, float *G)
{
    G[e] = gr;
    const float th = P[e];
    if (a.weight_decay != 0.f) gr = fmaf(a.weight_decay, th, gr);
    const float m = M[e] + (gr - M[e]) * a.one_minus_beta1;
    const float v = fmaf(a.one_minus_beta2 * gr, gr, V[e] * a.beta2);
    M[e] = m;
    V[e] = v;
    P[e] = th - a.step_size * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
}

constexpr int kEmbEntries = M6A_N_KMERS * 2;

// blocks [0, 132): a wave per embedding entry; the others: a thread per float of the blob behind the embedding
__global__ __launch_bounds__(64) void train_adam_kernel(Batch bt, const float *__restrict__ part, int n_chunks, const double *__restrict__ tot,
                                                        const float *__restrict__ dxe, AdamArgs a, float *__restrict__ P, float *__restrict__ M,
                                                        float *__restrict__ V, float *__restrict__ G)
{
    const int lane = threadIdx.x;
    if (blockIdx.x < kEmbEntries) {
        const int e = blockIdx.x, v = e >> 1, d = e & 1;
        double acc = 0.0;
        for (int64_t b = lane; b < bt.B; b += 64) {
            const int64_t site = bt.sidx ? bt.sidx[b] : b;
            for (int s = 0; s < 3; s++)
                if (bt.km[site * 3 + s] == v)
                    for (int k = 0; k < bt.bag; k++) acc += (double)dxe[(b * bt.bag + k) * 6 + 2 * s + d];
        }
        acc = wave_sum(acc);
        if (lane == 0) adam_apply(e, (float)acc, a, P, M, V, G);
        return;
    }
    const int e = kEmbEntries + (blockIdx.x - kEmbEntries) * 64 + lane;
    if (e >= M6A_N_WEIGHTS) return;
    if (e >= oMean && e < oW2) { G[e] = 0.f; return; }           // the running statistics are not parameters
    float gr;
    if (e >= oGamma && e < oBeta) gr = (float)tot[kH1 + e - oGamma];
    else if (e >= oBeta && e < oMean) gr = (float)tot[e - oBeta];
    else {
        double acc = 0.0;
        for (int c0 = 0; c0 < n_chunks; c0 += kBatch) {
            float v[kBatch];
            for (int u = 0; u < kBatch; u++) v[u] = c0 + u < n_chunks ? part[(size_t)(c0 + u) * M6A_N_WEIGHTS + e] : 0.f;
            for (int u = 0; u < kBatch; u++) if (c0 + u < n_chunks) acc += (double)v[u];
        }
        gr = (float)acc;
    }
    adam_apply(e, gr, a, P, M, V, G);
}

// ---- the step with gradient clipping: train_adam_kernel in two, because every block needs the whole gradient's norm ----------------
constexpr int kGradBlocks = kEmbEntries + (M6A_N_WEIGHTS - kEmbEntries + 63) / 64;      // the grid of train_adam_kernel
constexpr int kClipThreads = 256;

// The folds of train_adam_kernel on its grid, in its order; G = the gradient (unclipped), sq[block] = the block's sum of g^2 in
// float64: an embedding block has one value, the others the wave_sum butterfly of their 64 lanes' values.
__global__ __launch_bounds__(64) void train_grad_kernel(Batch bt, const float *__restrict__ part, int n_chunks, const double *__restrict__ tot,
                                                        const float *__restrict__ dxe, float *__restrict__ G, double *__restrict__ sq)
{
    const int lane = threadIdx.x;
    if (blockIdx.x < kEmbEntries) {
        const int e = blockIdx.x, v = e >> 1, d = e & 1;
        double acc = 0.0;
        for (int64_t b = lane; b < bt.B; b += 64) {
            const int64_t site = bt.sidx ? bt.sidx[b] : b;
            for (int s = 0; s < 3; s++)
                if (bt.km[site * 3 + s] == v)
                    for (int k = 0; k < bt.bag; k++) acc += (double)dxe[(b * bt.bag + k) * 6 + 2 * s + d];
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            const float gr = (float)acc;
            G[e] = gr;
            sq[e] = (double)gr * (double)gr;
        }
        return;
    }
    const int e = kEmbEntries + (blockIdx.x - kEmbEntries) * 64 + lane;
    float gr = 0.f;
    if (e < M6A_N_WEIGHTS && !(e >= oMean && e < oW2)) {          // the running statistics are not parameters: they count as 0
        if (e >= oGamma && e < oBeta) gr = (float)tot[kH1 + e - oGamma];
        else if (e >= oBeta && e < oMean) gr = (float)tot[e - oBeta];
        else {
            double acc = 0.0;
            for (int c0 = 0; c0 < n_chunks; c0 += kBatch) {
                float v[kBatch];
                for (int u = 0; u < kBatch; u++) v[u] = c0 + u < n_chunks ? part[(size_t)(c0 + u) * M6A_N_WEIGHTS + e] : 0.f;
                for (int u = 0; u < kBatch; u++) if (c0 + u < n_chunks) acc += (double)v[u];
            }
            gr = (float)acc;
        }
    }
    if (e < M6A_N_WEIGHTS) G[e] = gr;
    const double s = wave_sum((double)gr * (double)gr);           // every lane of the block is here
    if (lane == 0) sq[blockIdx.x] = s;
}

// A thread per float of the blob.  Every thread adds the kGradBlocks partial sums in block-index order, so all of them hold the same
// total = sqrt(sum g^2) and coef = min(1, max_norm / (total + 1e-6)) (torch.nn.utils.clip_grad_norm_, both float32); then
// g <- coef g (at coef = 1 no bit changes) and Adam.  *norm = total, from before the scaling.
__global__ __launch_bounds__(kClipThreads) void train_clip_adam_kernel(const double *__restrict__ sq, float max_norm, AdamArgs a,
                                                                       float *__restrict__ P, float *__restrict__ M, float *__restrict__ V,
                                                                       float *__restrict__ G, float *__restrict__ norm)
{
    __shared__ double sqs[kGradBlocks];                           // one global load per thread, then the ordered sum out of LDS
    for (int b = threadIdx.x; b < kGradBlocks; b += kClipThreads) sqs[b] = sq[b];
    __syncthreads();
    double acc = 0.0;
    for (int b = 0; b < kGradBlocks; b++) acc += sqs[b];
    const float total = (float)sqrt(acc);
    const float coef = fminf(max_norm / (total + 1e-6f), 1.0f);
    const int e = blockIdx.x * kClipThreads + threadIdx.x;
    if (e == 0) *norm = total;
    if (e >= M6A_N_WEIGHTS) return;
    if (e >= oMean && e < oW2) return;                            // G is 0 there already
    adam_apply(e, G[e] * coef, a, P, M, V, G);
}

}  // namespace

struct __attribute__((visibility("hidden"))) m6a_trainer {                 // its destructor (the DevBufs') is no symbol of the library
    m6a_ctx *c = nullptr;
    m6a_train_config cfg{};
    float *P = nullptr, *M = nullptr, *V = nullptr, *G = nullptr;       // [M6A_N_WEIGHTS] each, blob order
    double *stat = nullptr, *tot = nullptr, *part1 = nullptr;           // [300], [300], [kMaxChunks][300]
    float *part2 = nullptr;                                             // [kMaxChunks][M6A_N_WEIGHTS]
    unsigned long long *d_err = nullptr, *h_err = nullptr;
    DevBuf z1, dy1, xbuf, h2, dlogit, dxe, wpart, loss_term, ridx;      // scratch, sized for the largest batch seen
    DevBuf sX, sK, sOff, sY, sOrder, sLoss, sPred;                      // host-pointer calls
    double *sq = nullptr;                                               // [kGradBlocks] sums of g^2 (clipping)
    float *norm = nullptr;                                              // the last clipped step's total norm
    float clip = 0.f;                                                   // max_norm, 0 = no clipping
    bool have_norm = false;
    int64_t n_steps = 0, n_launches = 0, n_syncs = 0;
    // m6a_train_forward / m6a_train_backward: the latest forward's activations live in z1, xbuf, h2 and stat, its k-mers in keptK
    DevBuf keptK, sGradS;
    int64_t n_forwards = 0, kept_ticket = 0, kept_B = 0;                // kept_ticket 0: nothing is kept
    int kept_bag = 0;
    const char *kept_lost = "no forward has been made on this trainer";
};

namespace {

int ensure_scratch(m6a_trainer *t, int64_t B, int bag)
{
    m6a_ctx *c = t->c;
    const size_t N = (size_t)B * bag;
    const size_t n_waves = (size_t)((B + 64 / bag - 1) / (64 / bag));
    if (N * kH1 * 4 > t->z1.cap || N * kXs * 4 > t->xbuf.cap || N * kH2 * 4 > t->h2.cap) {      // what m6a_train_backward reads again
        t->kept_ticket = 0;
        t->kept_lost = "a larger batch on this trainer made it allocate its scratch anew";
    }
    HIPCHK(c, t->z1.ensure(N * kH1 * 4));
    HIPCHK(c, t->dy1.ensure(N * kH1 * 4));
    HIPCHK(c, t->xbuf.ensure(N * kXs * 4));
    HIPCHK(c, t->h2.ensure(N * kH2 * 4));
    HIPCHK(c, t->dlogit.ensure(N * 4));
    HIPCHK(c, t->dxe.ensure(N * 6 * 4));
    HIPCHK(c, t->wpart.ensure(n_waves * 2 * kH1 * 4));
    HIPCHK(c, t->loss_term.ensure((size_t)B * 4));
    return M6A_OK;
}

// after the check kernels' launches: reads the lowest (index, kind) they reported; one wait for the stream
int checked(m6a_trainer *t)
{
    m6a_ctx *c = t->c;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(t->h_err, t->d_err, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t->n_syncs++;
    const unsigned long long e = *t->h_err;
    if (e == ~0ull) return M6A_OK;
    const long long at = (long long)(e >> 3);
    switch ((int)(e & 7)) {
    case kErrReads: return fail(c, M6A_EINVAL, "site %lld has fewer reads than bag (or more than 2^32 - 1)", at);
    case kErrKmer: return fail(c, M6A_EINVAL, "site %lld: k-mer id outside 0..%d", at, M6A_N_KMERS - 1);
    case kErrLabel: return fail(c, M6A_EINVAL, "site %lld: the label is not 0 or 1", at);
    default: return fail(c, M6A_EINVAL, "order[%lld] is outside [0, n_sites)", at);
    }
}

// how a batch is cut: chunks of whole 32-read tiles for layer 1 and its backward, 64 / bag whole bags per wave for train_fwd2_kernel
struct Cut { int64_t chunk, n_waves; int n_chunks, per_wave; };

Cut cut(const Batch &bt)
{
    Cut k;
    k.chunk = (bt.N + kMaxChunks - 1) / kMaxChunks;
    k.chunk = std::max<int64_t>(kTile, (k.chunk + kTile - 1) / kTile * kTile);
    k.n_chunks = (int)((bt.N + k.chunk - 1) / k.chunk);
    k.per_wave = 64 / bt.bag;
    k.n_waves = (bt.B + k.per_wave - 1) / k.per_wave;
    return k;
}

// queues one step; every pointer is a device pointer and the scratch is large enough
int queue_step(m6a_trainer *t, const Batch &bt, float *loss, float *y_pred)
{
    m6a_ctx *c = t->c;
    hipStream_t st = c->stream;
    const int64_t N = bt.N;
    const Cut k = cut(bt);
    const int64_t chunk = k.chunk, n_waves = k.n_waves;
    const int n_chunks = k.n_chunks, per_wave = k.per_wave;
    float *z1 = (float *)t->z1.p, *dy1 = (float *)t->dy1.p, *xbuf = (float *)t->xbuf.p, *h2 = (float *)t->h2.p, *dl = (float *)t->dlogit.p,
          *dxe = (float *)t->dxe.p, *wpart = (float *)t->wpart.p, *lt = (float *)t->loss_term.p;
    t->n_steps++;
    t->kept_ticket = 0;
    t->kept_lost = "a step or an epoch on this trainer overwrote those activations";
    const double b1 = t->cfg.beta1, b2 = t->cfg.beta2;
    AdamArgs a;
    a.step_size = (float)((double)t->cfg.lr / (1.0 - std::pow(b1, (double)t->n_steps)));
    a.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, (double)t->n_steps));
    a.beta1 = t->cfg.beta1; a.beta2 = t->cfg.beta2;
    a.one_minus_beta1 = (float)(1.0 - b1); a.one_minus_beta2 = (float)(1.0 - b2);
    a.eps = t->cfg.eps; a.weight_decay = t->cfg.weight_decay;

    hipLaunchKernelGGL(train_fwd1_kernel, dim3((unsigned)n_chunks), dim3(192), 0, st, bt, chunk, (const float *)t->P, xbuf, z1, t->part1);
    hipLaunchKernelGGL(train_stats_kernel, dim3(1), dim3(192), 0, st, (const double *)t->part1, n_chunks, N, t->P, t->stat);
    hipLaunchKernelGGL(train_fwd2_kernel<kFused>, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, st, bt, per_wave, n_waves, 1.0f / (float)bt.B,
                       (const float *)z1, (const double *)t->stat, (const float *)t->P, h2, dl, dy1, wpart, lt, y_pred);
    hipLaunchKernelGGL(train_fold_kernel, dim3(1), dim3(256), 0, st, (const float *)wpart, n_waves, t->tot, (const float *)lt, bt.B, loss);
    hipLaunchKernelGGL(train_bwd1_kernel, dim3((unsigned)n_chunks), dim3(192), 0, st, N, chunk, (const float *)z1, (const float *)dy1,
                       (const float *)xbuf, (const float *)h2, (const float *)dl, (const double *)t->stat, (const double *)t->tot,
                       (const float *)t->P, t->part2, dxe);
    if (t->clip > 0.f) {
        hipLaunchKernelGGL(train_grad_kernel, dim3(kGradBlocks), dim3(64), 0, st, bt, (const float *)t->part2, n_chunks, (const double *)t->tot,
                           (const float *)dxe, t->G, t->sq);
        hipLaunchKernelGGL(train_clip_adam_kernel, dim3((M6A_N_WEIGHTS + kClipThreads - 1) / kClipThreads), dim3(kClipThreads), 0, st,
                           (const double *)t->sq, t->clip, a, t->P, t->M, t->V, t->G, t->norm);
        t->have_norm = true;
        t->n_launches += 7;
    } else {
        hipLaunchKernelGGL(train_adam_kernel, dim3(kGradBlocks), dim3(64), 0, st, bt, (const float *)t->part2, n_chunks, (const double *)t->tot,
                           (const float *)dxe, a, t->P, t->M, t->V, t->G);
        t->n_launches += 6;
    }
    HIPCHK(c, hipGetLastError());
    return M6A_OK;
}

// the context's prologue (m6a_ctx.h) behind a trainer; the device is selected at once: every trainer call works on it
int enter(m6a_trainer *t)
{
    if (!t) return M6A_EINVAL;
    int rc = m6a_detail::enter(t->c);
    if (rc) return rc;
    HIPCHK(t->c, hipSetDevice(t->c->device));
    return M6A_OK;
}

// the closing synchronise of a call that hands results to the host, counted for m6a_train_stats
int sync_counted(m6a_trainer *t)
{
    HIPCHK(t->c, hipStreamSynchronize(t->c->stream));
    t->n_syncs++;
    return M6A_OK;
}

int copy_out(m6a_trainer *t, void *dst, const void *src, size_t bytes)
{
    HIPCHK(t->c, hipMemcpyAsync(dst, src, bytes, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, t->c->stream));
    return sync_counted(t);
}

}  // namespace

extern "C" {

int m6a_train_create(m6a_ctx *c, const float *weights, size_t n_floats, const m6a_train_config *cfg, m6a_trainer **out)
{
    if (!c || !out) return M6A_EINVAL;
    *out = nullptr;
    settle(c);
    if (!weights || n_floats != M6A_N_WEIGHTS) return fail(c, M6A_EINVAL, "weights must be %d floats", M6A_N_WEIGHTS);
    if (is_device_ptr(weights)) return fail(c, M6A_EINVAL, "weights is a host pointer");
    m6a_train_config k = {4e-4f, 0.9f, 0.999f, 1e-8f, 0.f};
    if (cfg) k = *cfg;
    if (!(k.lr >= 0.f) || !(k.beta1 >= 0.f && k.beta1 < 1.f) || !(k.beta2 >= 0.f && k.beta2 < 1.f) || !(k.eps >= 0.f) || !(k.weight_decay >= 0.f))
        return fail(c, M6A_EINVAL, "m6a_train_config: lr, eps, weight_decay >= 0 and 0 <= beta < 1 (torch.optim.Adam's conditions)");
    HIPCHK(c, hipSetDevice(c->device));
    m6a_trainer *t = new (std::nothrow) m6a_trainer;
    if (!t) return fail(c, M6A_ENOMEM, "out of host memory");
    t->c = c;
    t->cfg = k;
    const size_t wb = (size_t)M6A_N_WEIGHTS * 4;
    hipError_t e = hipMalloc((void **)&t->P, 4 * wb);
    if (e == hipSuccess) e = hipMalloc((void **)&t->stat, ((size_t)(2 + kMaxChunks) * 2 * kH1 + kGradBlocks + 1) * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&t->part2, (size_t)kMaxChunks * wb);
    if (e == hipSuccess) e = hipMalloc((void **)&t->d_err, 8);
    if (e == hipSuccess) e = hipHostMalloc((void **)&t->h_err, 8);
    if (e == hipSuccess) e = hipMemsetAsync(t->P, 0, 4 * wb, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->P, weights, wb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        m6a_train_destroy(t);
        return fail(c, e == hipErrorOutOfMemory ? M6A_ENOMEM : M6A_EHIP, "m6a_train_create: %s", hipGetErrorString(e));
    }
    t->M = t->P + M6A_N_WEIGHTS; t->V = t->M + M6A_N_WEIGHTS; t->G = t->V + M6A_N_WEIGHTS;
    t->tot = t->stat + 2 * kH1; t->part1 = t->tot + 2 * kH1;
    t->sq = t->part1 + (size_t)kMaxChunks * 2 * kH1; t->norm = (float *)(t->sq + kGradBlocks);
    *out = t;
    return M6A_OK;
}

void m6a_train_destroy(m6a_trainer *t)
{
    if (!t) return;
    if (t->c) { (void)hipSetDevice(t->c->device); (void)hipStreamSynchronize(t->c->stream); }
    if (t->P) (void)hipFree(t->P);
    if (t->stat) (void)hipFree(t->stat);
    if (t->part2) (void)hipFree(t->part2);
    if (t->d_err) (void)hipFree(t->d_err);
    if (t->h_err) (void)hipHostFree(t->h_err);
    delete t;                                           // with every DevBuf it holds
}

int m6a_train_step(m6a_trainer *t, const float *X, const uint8_t *km, const float *y, int64_t B, int bag, float *loss, float *y_pred)
{
    int rc = enter(t);
    if (rc) return rc;
    m6a_ctx *c = t->c;
    if (bag < 1 || bag > M6A_MAX_SAMPLES) return fail(c, M6A_EINVAL, "bag must be in 1..%d", M6A_MAX_SAMPLES);
    if (B < 1 || B * bag < 2) return fail(c, M6A_EINVAL, "a step needs n_bags * bag >= 2 reads (batch norm over one value is undefined)");
    if (B > kMaxBatchReads || B * bag > kMaxBatchReads) return fail(c, M6A_EINVAL, "a batch holds at most 2^20 reads");
    if (!X || !km || !y) return fail(c, M6A_EINVAL, "null pointer argument");
    const int dev = same_side(c, X, {km, y, loss, y_pred}, "X, site_kmers, y, loss, y_pred must be all host or all device pointers");
    if (dev < 0) return dev;
    const int64_t N = B * bag;
    rc = ensure_scratch(t, B, bag);
    if (rc) return rc;
    HIPCHK(c, t->sLoss.ensure(4));
    HIPCHK(c, t->sPred.ensure((size_t)B * 4));
    Batch bt{X, nullptr, km, nullptr, y, B, N, bag};
    if (!dev) {
        HIPCHK(c, stage_in(c, t->sX, X, (size_t)N * 9 * 4));
        HIPCHK(c, stage_in(c, t->sK, km, (size_t)B * 3));
        HIPCHK(c, stage_in(c, t->sY, y, (size_t)B * 4));
        bt.X = (const float *)t->sX.p; bt.km = (const uint8_t *)t->sK.p; bt.y = (const float *)t->sY.p;
    }
    HIPCHK(c, hipMemsetAsync(t->d_err, 0xff, 8, c->stream));       // nothing reported yet (checked)
    hipLaunchKernelGGL(train_check_sites_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, bt.km, (const int64_t *)nullptr, bt.y,
                       B, bag, t->d_err);
    t->n_launches++;
    rc = checked(t);
    if (rc) return rc;
    float *d_loss = dev && loss ? loss : (float *)t->sLoss.p, *d_pred = dev && y_pred ? y_pred : (float *)t->sPred.p;
    rc = queue_step(t, bt, d_loss, d_pred);
    if (rc || dev) return rc;
    if (loss) HIPCHK(c, stage_out(c, loss, t->sLoss, 4));
    if (y_pred) HIPCHK(c, stage_out(c, y_pred, t->sPred, (size_t)B * 4));
    return sync_counted(t);
}

int m6a_train_epoch(m6a_trainer *t, const float *X, const uint8_t *km, const int64_t *off, const float *y, int64_t S, const int64_t *order,
                    int64_t n_order, int64_t bs, int bag, uint64_t seed, float *loss, float *y_pred)
{
    int rc = enter(t);
    if (rc) return rc;
    m6a_ctx *c = t->c;
    if (bag < 1 || bag > M6A_MAX_SAMPLES) return fail(c, M6A_EINVAL, "bag must be in 1..%d", M6A_MAX_SAMPLES);
    if (S < 1 || n_order < 0 || bs < 1) return fail(c, M6A_EINVAL, "n_sites >= 1, n_order >= 0 and batch_size >= 1");
    if (n_order == 0) return M6A_OK;
    const int64_t largest = std::min(bs, n_order), last = n_order % bs ? n_order % bs : largest;
    if (largest > kMaxBatchReads || largest * bag > kMaxBatchReads) return fail(c, M6A_EINVAL, "a batch holds at most 2^20 reads");
    if (last * bag < 2) return fail(c, M6A_EINVAL, "a batch of this epoch has fewer than 2 reads (batch norm over one value is undefined)");
    if (n_order > INT64_MAX / 8 / bag) return fail(c, M6A_EINVAL, "n_order * bag too large");
    if (!X || !km || !off || !y || !order) return fail(c, M6A_EINVAL, "null pointer argument");
    const int dev = same_side(c, X, {km, off, y, order, loss, y_pred},
                              "X, site_kmers, off, y, order, loss, y_pred must be all host or all device pointers");
    if (dev < 0) return dev;
    const int64_t n_steps = (n_order + bs - 1) / bs;
    rc = ensure_scratch(t, largest, bag);
    if (rc) return rc;
    HIPCHK(c, t->ridx.ensure((size_t)n_order * bag * 8));
    HIPCHK(c, t->sLoss.ensure((size_t)n_steps * 4));
    HIPCHK(c, t->sPred.ensure((size_t)n_order * 4));
    const int64_t *d_off = off, *d_order = order;
    Batch bt{X, nullptr, km, nullptr, y, 0, 0, bag};
    if (!dev) {
        // a host dataset goes up once per call
        rc = csr_check(c, off, S);
        if (rc) return rc;
        HIPCHK(c, stage_in(c, t->sX, X, (size_t)off[S] * 9 * 4));
        HIPCHK(c, stage_in(c, t->sK, km, (size_t)S * 3));
        HIPCHK(c, stage_in(c, t->sOff, off, (size_t)(S + 1) * 8));
        HIPCHK(c, stage_in(c, t->sY, y, (size_t)S * 4));
        HIPCHK(c, stage_in(c, t->sOrder, order, (size_t)n_order * 8));
        bt.X = (const float *)t->sX.p; bt.km = (const uint8_t *)t->sK.p; bt.y = (const float *)t->sY.p;
        d_off = (const int64_t *)t->sOff.p; d_order = (const int64_t *)t->sOrder.p;
    }
    int64_t *ridx = (int64_t *)t->ridx.p;
    HIPCHK(c, hipMemsetAsync(t->d_err, 0xff, 8, c->stream));       // nothing reported yet (checked)
    hipLaunchKernelGGL(train_check_sites_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, c->stream, bt.km, d_off, bt.y, S, bag, t->d_err);
    hipLaunchKernelGGL(train_draw_kernel, dim3((unsigned)((n_order + 63) / 64)), dim3(64), 0, c->stream, d_off, d_order, n_order, S, bag, seed, ridx,
                       t->d_err);
    t->n_launches += 2;
    rc = checked(t);
    if (rc) return rc;
    float *d_loss = dev && loss ? loss : (float *)t->sLoss.p, *d_pred = dev && y_pred ? y_pred : (float *)t->sPred.p;
    for (int64_t k = 0; k < n_steps; k++) {             // queued back to back: nothing below waits for the device
        bt.B = std::min(bs, n_order - k * bs);
        bt.N = bt.B * bag;
        bt.ridx = ridx + k * bs * bag;
        bt.sidx = d_order + k * bs;
        rc = queue_step(t, bt, d_loss + k, d_pred + k * bs);
        if (rc) return rc;
    }
    if (dev) return M6A_OK;
    if (loss) HIPCHK(c, stage_out(c, loss, t->sLoss, (size_t)n_steps * 4));
    if (y_pred) HIPCHK(c, stage_out(c, y_pred, t->sPred, (size_t)n_order * 4));
    return sync_counted(t);
}

// ---- the step cut at s: forward gives s, backward takes dL/ds (include/m6a.h) -------------------------------------------------------
int m6a_train_set_weights(m6a_trainer *t, const float *blob)
{
    int rc = enter(t);
    if (rc) return rc;
    m6a_ctx *c = t->c;
    if (!blob) return fail(c, M6A_EINVAL, "null pointer argument");
    const bool dev = is_device_ptr(blob);
    HIPCHK(c, hipMemcpyAsync(t->P, blob, (size_t)M6A_N_WEIGHTS * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    t->kept_ticket = 0;
    t->kept_lost = "the weights were replaced since that forward (m6a_train_set_weights)";
    return dev ? M6A_OK : sync_counted(t);
}

int m6a_train_running_stats(m6a_trainer *t, float *stats)
{
    int rc = enter(t);
    if (rc) return rc;
    m6a_ctx *c = t->c;
    if (!stats) return fail(c, M6A_EINVAL, "null pointer argument");
    if (!is_device_ptr(stats)) return copy_out(t, stats, t->P + oMean, (size_t)2 * kH1 * 4);
    HIPCHK(c, hipMemcpyAsync(stats, t->P + oMean, (size_t)2 * kH1 * 4, hipMemcpyDeviceToDevice, c->stream));
    return M6A_OK;
}

int m6a_train_forward(m6a_trainer *t, const float *X, const uint8_t *km, int64_t B, int bag, int training, float *s, int64_t *ticket)
{
    int rc = enter(t);
    if (rc) return rc;
    m6a_ctx *c = t->c;
    if (!training) return fail(c, M6A_EINVAL, "training = 0: the trainer runs batch norm on the batch's statistics only; eval mode is m6a_bag_forward's");
    if (bag < 1 || bag > M6A_MAX_SAMPLES) return fail(c, M6A_EINVAL, "bag must be in 1..%d", M6A_MAX_SAMPLES);
    if (B < 1 || B * bag < 2) return fail(c, M6A_EINVAL, "a forward needs n_bags * bag >= 2 reads (batch norm over one value is undefined)");
    if (B > kMaxBatchReads || B * bag > kMaxBatchReads) return fail(c, M6A_EINVAL, "a batch holds at most 2^20 reads");
    if (!X || !km || !s || !ticket) return fail(c, M6A_EINVAL, "null pointer argument");
    const int dev = same_side(c, X, {km, s}, "X, site_kmers, s must be all host or all device pointers");
    if (dev < 0) return dev;
    const int64_t N = B * bag;
    const uint8_t *d_km = km;
    if (!dev) {
        HIPCHK(c, stage_in(c, t->sK, km, (size_t)B * 3));
        d_km = (const uint8_t *)t->sK.p;
    }
    HIPCHK(c, hipMemsetAsync(t->d_err, 0xff, 8, c->stream));       // nothing reported yet (checked)
    hipLaunchKernelGGL(train_check_kmers_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, d_km, B, t->d_err);
    t->n_launches++;
    rc = checked(t);
    if (rc) return rc;                                  // nothing is changed: an earlier forward's activations are still kept
    t->kept_ticket = 0;
    t->kept_lost = "a later forward on this trainer failed part-way";
    rc = ensure_scratch(t, B, bag);
    if (rc) return rc;
    HIPCHK(c, t->keptK.ensure((size_t)B * 3));
    HIPCHK(c, hipMemcpyAsync(t->keptK.p, d_km, (size_t)B * 3, hipMemcpyDeviceToDevice, c->stream));
    Batch bt{X, nullptr, (const uint8_t *)t->keptK.p, nullptr, nullptr, B, N, bag};
    float *d_s = s;
    if (!dev) {
        HIPCHK(c, t->sPred.ensure((size_t)B * 4));
        HIPCHK(c, stage_in(c, t->sX, X, (size_t)N * 9 * 4));
        bt.X = (const float *)t->sX.p;
        d_s = (float *)t->sPred.p;
    }
    const Cut k = cut(bt);
    hipStream_t st = c->stream;
    float *z1 = (float *)t->z1.p;
    hipLaunchKernelGGL(train_fwd1_kernel, dim3((unsigned)k.n_chunks), dim3(192), 0, st, bt, k.chunk, (const float *)t->P, (float *)t->xbuf.p, z1,
                       t->part1);
    hipLaunchKernelGGL(train_stats_kernel, dim3(1), dim3(192), 0, st, (const double *)t->part1, k.n_chunks, N, t->P, t->stat);
    hipLaunchKernelGGL(train_fwd2_kernel<kForward>, dim3((unsigned)((k.n_waves + 3) / 4)), dim3(256), 0, st, bt, k.per_wave, k.n_waves, 0.f,
                       (const float *)z1, (const double *)t->stat, (const float *)t->P, (float *)t->h2.p, (float *)nullptr, (float *)nullptr,
                       (float *)nullptr, (float *)nullptr, d_s);
    t->n_launches += 3;
    HIPCHK(c, hipGetLastError());
    t->kept_ticket = ++t->n_forwards;
    t->kept_B = B;
    t->kept_bag = bag;
    t->kept_lost = "a later forward on this trainer overwrote those activations";
    *ticket = t->kept_ticket;
    if (dev) return M6A_OK;
    HIPCHK(c, stage_out(c, s, t->sPred, (size_t)B * 4));
    return sync_counted(t);
}

int m6a_train_backward(m6a_trainer *t, int64_t ticket, const float *grad_s, float *grads)
{
    int rc = enter(t);
    if (rc) return rc;
    m6a_ctx *c = t->c;
    if (!grad_s || !grads) return fail(c, M6A_EINVAL, "null pointer argument");
    if (ticket < 1 || ticket > t->n_forwards) return fail(c, M6A_EINVAL, "ticket %lld was not given by m6a_train_forward on this trainer", (long long)ticket);
    if (ticket != t->kept_ticket) return fail(c, M6A_EINVAL, "the activations of ticket %lld are gone: %s", (long long)ticket, t->kept_lost);
    const int dev = same_side(c, grad_s, {grads}, "grad_s, grads must be all host or all device pointers");
    if (dev < 0) return dev;
    const int64_t B = t->kept_B;
    const float *d_g = grad_s;
    if (!dev) {
        HIPCHK(c, stage_in(c, t->sGradS, grad_s, (size_t)B * 4));
        d_g = (const float *)t->sGradS.p;
    }
    HIPCHK(c, t->sLoss.ensure(4));
    // the place of the labels holds dL/ds (train_fwd2_kernel<kBackward>); X is not read again: xbuf has the forward's gather
    Batch bt{nullptr, nullptr, (const uint8_t *)t->keptK.p, nullptr, d_g, B, B * t->kept_bag, t->kept_bag};
    const Cut k = cut(bt);
    hipStream_t st = c->stream;
    float *z1 = (float *)t->z1.p, *dy1 = (float *)t->dy1.p, *h2 = (float *)t->h2.p, *dl = (float *)t->dlogit.p, *dxe = (float *)t->dxe.p,
          *wpart = (float *)t->wpart.p;
    hipLaunchKernelGGL(train_fwd2_kernel<kBackward>, dim3((unsigned)((k.n_waves + 3) / 4)), dim3(256), 0, st, bt, k.per_wave, k.n_waves, 0.f,
                       (const float *)z1, (const double *)t->stat, (const float *)t->P, h2, dl, dy1, wpart, (float *)nullptr, (float *)nullptr);
    // B = 0 for the fold's loss wave: it adds nothing and its one store goes to scratch nobody reads -- the loss is the caller's
    hipLaunchKernelGGL(train_fold_kernel, dim3(1), dim3(256), 0, st, (const float *)wpart, k.n_waves, t->tot, (const float *)nullptr, (int64_t)0,
                       (float *)t->sLoss.p);
    hipLaunchKernelGGL(train_bwd1_kernel, dim3((unsigned)k.n_chunks), dim3(192), 0, st, bt.N, k.chunk, (const float *)z1, (const float *)dy1,
                       (const float *)t->xbuf.p, (const float *)h2, (const float *)dl, (const double *)t->stat, (const double *)t->tot,
                       (const float *)t->P, t->part2, dxe);
    hipLaunchKernelGGL(train_grad_kernel, dim3(kGradBlocks), dim3(64), 0, st, bt, (const float *)t->part2, k.n_chunks, (const double *)t->tot,
                       (const float *)dxe, t->G, t->sq);
    t->n_launches += 4;
    HIPCHK(c, hipGetLastError());
    if (!dev) return copy_out(t, grads, t->G, (size_t)M6A_N_WEIGHTS * 4);
    HIPCHK(c, hipMemcpyAsync(grads, t->G, (size_t)M6A_N_WEIGHTS * 4, hipMemcpyDeviceToDevice, c->stream));
    return M6A_OK;
}

int m6a_train_sample(const int64_t *off, const int64_t *order, int64_t n_order, int bag, uint64_t seed, int64_t *read_idx)
{
    if (!off || !order || !read_idx || n_order < 0 || bag < 1 || bag > M6A_MAX_SAMPLES) return M6A_EINVAL;
    for (int64_t i = 0; i < n_order; i++) {
        const int64_t s = order[i];
        if (s < 0) return M6A_EINVAL;
        const int64_t lo = off[s], n = off[s + 1] - lo;
        if (n < bag || n > 0xffffffffll) return M6A_EINVAL;
        int64_t out[m6a_train_draw::kMaxBag];
        m6a_train_draw::draw(seed, (uint64_t)i, (uint64_t)n, bag, out);
        for (int j = 0; j < bag; j++) read_idx[i * bag + j] = lo + out[j];
    }
    return M6A_OK;
}

int m6a_train_grads(m6a_trainer *t, float *grads)
{
    int rc = enter(t);
    if (rc) return rc;
    if (!grads) return fail(t->c, M6A_EINVAL, "null pointer argument");
    return copy_out(t, grads, t->G, (size_t)M6A_N_WEIGHTS * 4);
}

int m6a_train_weights(m6a_trainer *t, float *weights, int64_t *n_steps)
{
    int rc = enter(t);
    if (rc) return rc;
    if (n_steps) *n_steps = t->n_steps;
    if (!weights) return fail(t->c, M6A_EINVAL, "null pointer argument");
    return copy_out(t, weights, t->P, (size_t)M6A_N_WEIGHTS * 4);
}

int m6a_train_set_clip(m6a_trainer *t, float max_norm)
{
    int rc = enter(t);
    if (rc) return rc;
    if (!(max_norm >= 0.f) || std::isinf(max_norm)) return fail(t->c, M6A_EINVAL, "max_norm must be finite and >= 0 (0 = no clipping)");
    t->clip = max_norm;
    t->have_norm = false;
    return M6A_OK;
}

int m6a_train_last_norm(m6a_trainer *t, float *total_norm)
{
    int rc = enter(t);
    if (rc) return rc;
    if (!total_norm) return fail(t->c, M6A_EINVAL, "null pointer argument");
    if (!(t->clip > 0.f)) return fail(t->c, M6A_EINVAL, "clipping is off: the step does not compute the gradient's norm (m6a_train_set_clip)");
    if (!t->have_norm) return fail(t->c, M6A_EINVAL, "no step has been taken since clipping was set");
    return copy_out(t, total_norm, t->norm, 4);
}

int m6a_train_state_get(m6a_trainer *t, float *m, float *v, int64_t *n_steps)
{
    int rc = enter(t);
    if (rc) return rc;
    m6a_ctx *c = t->c;
    if (!m || !v) return fail(c, M6A_EINVAL, "null pointer argument");
    if (is_device_ptr(m) || is_device_ptr(v)) return fail(c, M6A_EINVAL, "m and v are host pointers");
    const size_t wb = (size_t)M6A_N_WEIGHTS * 4;
    HIPCHK(c, hipMemcpyAsync(m, t->M, wb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(v, t->V, wb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t->n_syncs++;
    if (n_steps) *n_steps = t->n_steps;
    return M6A_OK;
}

int m6a_train_state_set(m6a_trainer *t, const float *m, const float *v, int64_t n_steps)
{
    int rc = enter(t);
    if (rc) return rc;
    m6a_ctx *c = t->c;
    if (!m || !v) return fail(c, M6A_EINVAL, "null pointer argument");
    if (is_device_ptr(m) || is_device_ptr(v)) return fail(c, M6A_EINVAL, "m and v are host pointers");
    if (n_steps < 0) return fail(c, M6A_EINVAL, "n_steps must be >= 0");
    for (int e = 0; e < M6A_N_WEIGHTS; e++) {
        if (!std::isfinite(m[e])) return fail(c, M6A_EINVAL, "m[%d] is not finite", e);
        if (!(v[e] >= 0.f) || !std::isfinite(v[e])) return fail(c, M6A_EINVAL, "v[%d] is negative or not finite", e);
    }
    // staged, with the running-statistic slots at zero: they are not parameters and the kernels never touch them
    std::vector<float> mv((size_t)2 * M6A_N_WEIGHTS);
    std::copy(m, m + M6A_N_WEIGHTS, mv.begin());
    std::copy(v, v + M6A_N_WEIGHTS, mv.begin() + M6A_N_WEIGHTS);
    for (int e = oMean; e < oW2; e++) mv[e] = mv[M6A_N_WEIGHTS + e] = 0.f;
    HIPCHK(c, hipMemcpyAsync(t->M, mv.data(), mv.size() * 4, hipMemcpyHostToDevice, c->stream));    // M and V are adjacent
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t->n_syncs++;
    t->n_steps = n_steps;
    return M6A_OK;
}

int m6a_train_stats(const m6a_trainer *t, int64_t *n_steps, int64_t *n_launches, int64_t *n_syncs)
{
    if (!t) return M6A_EINVAL;
    if (n_steps) *n_steps = t->n_steps;
    if (n_launches) *n_launches = t->n_launches;
    if (n_syncs) *n_syncs = t->n_syncs;
    return M6A_OK;
}

}  // extern "C"
