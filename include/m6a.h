/*
 * m6a.h -- C ABI of libm6a_hip.so: m6anet's inference hot path on MI355X (gfx950).
 *
 * The reference (GoekeLab/m6anet) is pure Python and has no FFI; its seams for this path are
 * Python call sites.  Each entry point below names the reference interface it replaces
 * (paths relative to the reference checkout).  INTEGRATION.md shows the ctypes binding a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns M6A_OK (0) or a negative M6A_E* code; m6a_last_error(ctx) gives text;
 *   - the caller owns every buffer; the library keeps no input pointer after a call returns (one exception, stated
 *     there: DEVICE batches of a streaming job are read in place until m6a_job_end / m6a_job_abort);
 *   - DATA POINTERS of one call are all HOST or all DEVICE pointers (detected with hipPointerGetAttributes; an optional pointer
 *     that is NULL takes no side).  A mixture, a required pointer that is NULL, and a host off[] that does not start at 0 or
 *     decreases are M6A_EINVAL before anything is queued.  Where an argument is always a host array, its entry says so:
 *       all-host   -> the library stages through its own device buffers and the call is
 *                     synchronous (results are in the host buffers on return);
 *       all-device -> kernels are enqueued on the context's stream (m6a_set_stream); the
 *                     caller synchronises (m6a_sync or its own stream sync).  Entry points
 *                     read back a few bytes first (off[S]; min/max bag size to choose the
 *                     sampling kernel) and so block on the stream once or twice per call;
 *   - one ctx per (process, GPU, stream); calls on one ctx are not thread-safe;
 *   - no exceptions, no callbacks, no torch types cross this boundary (one exception, stated there: m6a_prep_sites_build calls
 *     the plain C functions of libm6a_io.so it is given for the runs its device front half declines).
 */
#ifndef M6A_H
#define M6A_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct m6a_ctx m6a_ctx;

enum {
    M6A_OK = 0,
    M6A_EINVAL = -1,     /* bad argument */
    M6A_ENOMEM = -2,     /* host or device allocation failed */
    M6A_EHIP = -3,       /* HIP runtime error (text in m6a_last_error) */
    M6A_ESTREAM = -4,    /* a flush group needs more MT19937 words than the stream cap allows */
    M6A_ENODEV = -5,     /* no usable gfx950 device */
    M6A_EUNSUPPORTED = -6,
    M6A_EFORMAT = -7,    /* malformed input file (m6a_prep_eventalign) */
    M6A_EIO = -8,        /* a file cannot be opened, read or written (m6a_prep_*) */
    M6A_EDECLINED = -9   /* the device CSV writer met a value it does not format; nothing was written (m6a_csv_format) */
};

/* rng_mode of m6a_site_pool / m6a_infer / m6a_job_begin.  M6A_RNG_NUMPY is the ONLY value: exact replay of the reference's
 * NumPy MT19937 stream -- the only sampler the reference has (np.random.choice at m6anet/utils/inference_utils.py:85, seeded at
 * scripts/inference.py:86).  The parameter stays in the three signatures because SURVEY.md section 8(b) fixed them; any other
 * value is M6A_EINVAL (a bad argument, not a missing feature: no counter-based mode is planned -- it could not meet the 1e-5
 * bar against the reference's draws, and indices are table reads in both pooling kernels, so it would not be faster either;
 * DESIGN.md section 8). */
enum { M6A_RNG_NUMPY = 0 };

#define M6A_N_WEIGHTS 7997
#define M6A_N_FEATURES 9     /* [dwell, std, mean] x {-1,0,+1}: DeaggregateNanopolish, blocks.py:113 */
#define M6A_MAX_SAMPLES 64
#define M6A_N_REPR 32        /* floats of the read representation: the width of the encoder's second layer (m6anet.toml:23-28) */
#define M6A_N_KMERS 66       /* vocabulary of 5-mers the DRACH 7-mers are made of (constants.py:29-36): k-mer ids are 0..65 */

/* Flat float32 weight blob, in this order (state-dict keys of m6anet/model/model.py:40-69,
 * files under m6anet/model/model_states/):
 *   E[66][2] | W1[150][15] | b1[150] | bn_gamma[150] | bn_beta[150] | bn_mean[150] | bn_var[150]
 *   | W2[32][150] | b2[32] | W3[32] | b3[1]                                     = 7997 floats.
 * Replaces: MILModel(...).load_state_dict(torch.load(...)) at m6anet/scripts/inference.py:88-90.
 * `weights` is a host pointer.  The weights are laid out for the kernels here; BatchNorm (eval, eps 1e-5) becomes the
 * (alpha, beta) = (gamma / sqrt(var + eps), fma(-mean, alpha, bias)) pair torch forms, applied per read in the kernel as
 * torch applies it -- nothing is folded into W1: the encoder's float32 sums run in the reference's order.
 * M6A_EUNSUPPORTED for a layer-2 weight or bias of magnitude >= 2^63 (the kernels carry them scaled by 2^64).
 * Which blobs the bit-for-bit claim of the 16-slot kernels (m6a_set_encoder_variant) covers -- any finite blob, trained here or
 * elsewhere, for which
 *   - every hidden activation relu(fma(z1, alpha, beta)) stays below 2^64 (the kernels hold it scaled by 2^-64 under a clamp to
 *     [0, 1]: beyond 2^64 it saturates there where the reference carries it on);
 *   - every alpha and beta above is 0 or at least 2^-62 in magnitude (smaller ones lose low bits in that scaling);
 *   - every layer-2 weight and bias stays below 2^63 in magnitude (refused above).
 * Inside that domain nothing else is asked of the weights: any sign, any zero (a gamma of 0 prunes its unit), running_var down
 * to 0 (alpha = gamma / sqrt(1e-5f), about 316 gamma).  A NaN weight gives NaN wherever the reference's arithmetic gives NaN.
 * tests/weight_families.py generates blobs across this domain; tests/test_gpu_encoder_weights.py runs every kernel on them. */
int m6a_create(m6a_ctx **out, const float *weights, size_t n_floats, int device_id);
void m6a_destroy(m6a_ctx *ctx);
const char *m6a_last_error(const m6a_ctx *ctx);   /* ctx may be NULL: last create error */

/* Use the caller's HIP stream (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream).
 * NULL selects the context's own stream. */
int m6a_set_stream(m6a_ctx *ctx, void *hip_stream);
/* Multi-GPU sharding: the sites passed to m6a_site_pool / m6a_infer on this context are sites
 * [first_site, first_site + n_sites) of a larger job.  Batch indices, hence flush groups and RNG
 * restarts (inference_utils.py:33,47), are counted from the job's first site, so results do not
 * depend on how the job is cut.  first_site must start a flush group (m6a_shard_plan returns
 * such cuts).  Default 0. */
int m6a_set_job_offset(m6a_ctx *ctx, int64_t first_site);
int m6a_sync(m6a_ctx *ctx);    /* waits for the stream; returns a deferred kernel-side error if any */
/* Optional, for calls with DEVICE pointers: hand over the host copy of the NEXT call's off[] (S+1 values; the loader that
 * built the CSR array has it -- the reference's collate keeps n_reads on the host, data_utils.py:498-506).  The bag
 * statistics that choose the kernels then come from this copy and the call neither reads anything back nor blocks on the
 * stream: consecutive calls queue back to back.  The device array is still checked against the copy, on the device; a
 * mismatch makes the results of that call undefined and is reported as a deferred M6A_EINVAL by the next m6a_sync.
 * One-shot: consumed by the next m6a_encode_reads / m6a_site_pool / m6a_infer / m6a_validate call on this context; the
 * pointer is read inside that call only.  NULL withdraws it. */
int m6a_set_host_offsets(m6a_ctx *ctx, const int64_t *off_host);
/* Optional: set up the host-pointer path now (pinned staging ring + copy threads; tens of milliseconds of page
 * pinning) instead of inside the first call that passes host buffers -- e.g. while the caller is still parsing
 * its input.  Host-buffer calls to m6a_infer / m6a_encode_reads cut the job into chunks and overlap the PCIe
 * transfer of chunk k+1 with the encoder of chunk k (the shape of the reference's batch loop,
 * m6anet/utils/inference_utils.py:33-41, without its per-batch synchronisation).  Pageable buffers pass through the ring
 * (copy threads + DMA); buffers the caller has page-locked (hipHostMalloc / hipHostRegister, torch's pin_memory()) are recognised
 * with hipPointerGetAttributes and DMA'd in place, chunk by chunk, in both directions -- same chunks, same kernels, same bits. */
int m6a_prepare_host_io(m6a_ctx *ctx);
/* Page-locked host memory (hipHostMalloc / hipHostFree) for callers with no other way to get it -- plain C, Python without
 * torch: buffers from m6a_host_alloc are DMA'd in place by the host-pointer calls above.  No context needed (the HIP runtime
 * must see a device).  Returns M6A_OK, M6A_ENOMEM or M6A_EHIP.  The reference's counterpart: DataLoader(pin_memory=...) is not
 * used by m6anet/utils/data_utils.py -- its batches are pageable. */
int m6a_host_alloc(size_t bytes, void **out);
int m6a_host_free(void *p);
/* 1 if the WHOLE range [p, p + bytes) lies inside ONE page-locked host allocation the DMA engines can address (hipHostMalloc,
 * hipHostRegister, torch's pin_memory(), m6a_host_alloc) -- exactly the test the host-pointer calls apply to decide between
 * in-place DMA and the staging ring; 0 otherwise (pageable memory, device memory, a range that leaves its allocation or spans
 * two registrations, no HIP runtime).  Never an error: a buffer that is not recognised simply goes through the ring. */
int m6a_host_is_pinned(const void *p, size_t bytes);

/* Read encoder.  Replaces, for one batch of sites,
 *     model.get_read_representation({'X','kmer'}) + model.pooling_filter.probability_layer(.)
 * (m6anet/utils/inference_utils.py:35-37 -> m6anet/model/model.py:85-97,
 *  m6anet/model/model_blocks/blocks.py:116-126,194-205,55-66,257-266, pooling_blocks.py:52).
 *   X          [R][9] float32, already z-normalised (data_utils.py:216-218)
 *   site_kmers [S][3] uint8 vocabulary ids 0..65 of the three 5-mers (stored once per site;
 *              the reference repeats them per read as int64, data_utils.py:223-224)
 *   off        [S+1] int64 CSR read offsets, off[0]=0, off[S]=R (the reference's n_reads vector,
 *              data_utils.py:499)
 *   read_prob  [R] float32 out */
int m6a_encode_reads(m6a_ctx *ctx, const float *X, const uint8_t *site_kmers, const int64_t *off,
                     int64_t n_sites, float *read_prob);

/* The read representation.  Replaces MILModel.get_read_representation({'X','kmer'}) (m6anet/model/model.py:85-97) on the
 * m6anet.toml topology: the output of the encoder's second layer after its ReLU,
 *     repr[r][o] = relu(b2[o] + sum_k W2[o][k] * relu(batchnorm(b1[k] + sum_j W1[k][j] * [x(9) | emb(6)][j]))),   o = 0..31,
 * every float32 sum in the order the reference's CPU arithmetic runs it (an fma chain over j, then + b1; one fma for the
 * batch norm; an fma chain over k = 0..149, then + b2: the order stated above enc_kernel in m6a_kernels.hip), so the
 * values are the reference's bits.  relu keeps NaN, as torch's does.
 *   X, site_kmers, off, n_sites  as m6a_encode_reads takes and checks them (m6a_set_host_offsets is consumed; n_sites == 0
 *              is M6A_OK with nothing written)
 *   repr       [R][M6A_N_REPR] float32 out, row r = read r, unit o at repr[r * 32 + o]; NULL is M6A_EINVAL and nothing is
 *              launched; a device pointer must be 16-byte aligned
 *   read_prob  [R] float32 out, or NULL: what m6a_encode_reads gives with the default encoder, bit for bit
 * The arithmetic does not depend on m6a_set_encoder_variant or M6A_ENCODER: one kernel (enc_repr_kernel) serves every bag
 * size.  Device pointers: queued on the context's stream.  Host pointers: the job is cut into chunks at site boundaries;
 * each chunk is uploaded, encoded and copied back in order on the context's stream (plain copies, not the pinned ring of
 * m6a_encode_reads: 128 bytes per read come back); the call returns when repr is complete. */
int m6a_read_representation(m6a_ctx *ctx, const float *X, const uint8_t *site_kmers, const int64_t *off,
                            int64_t n_sites, float *repr, float *read_prob);

/* m6a_read_representation with an output type.
 *   dtype      M6A_REPR_F32: repr is [R][M6A_N_REPR] float32 and the call is m6a_read_representation, bit for bit.
 *              M6A_REPR_F16: repr is [R][M6A_N_REPR] IEEE binary16, unit o of read r at ((uint16_t *)repr)[r * 32 + o]: the float32
 *              value the other form stores, converted once with round-to-nearest-even -- np.float32(v).astype(np.float16)
 *              exactly: NaN stays NaN, what rounds above 65504 is +inf, results in the binary16 subnormal range (below 2^-14)
 *              are produced, not flushed, and a value at or below 2^-25 is 0.  The kernel (enc_repr_kernel<true>) converts in
 *              registers and stores 32 contiguous bytes per lane; the float32 array is never written.
 *              Any other value is M6A_EINVAL and nothing is launched.
 *   repr       a device pointer must be 16-byte aligned (either type); host pointers go through m6a_read_representation's
 *              chunk loop, and 64 bytes per read come back with M6A_REPR_F16
 *   read_prob  unchanged by dtype: float32 [R] or NULL
 * Every other argument, check and error is m6a_read_representation's. */
#define M6A_REPR_F32 0
#define M6A_REPR_F16 1
int m6a_read_representation_dtype(m6a_ctx *ctx, const float *X, const uint8_t *site_kmers, const int64_t *off,
                                  int64_t n_sites, void *repr, int dtype, float *read_prob);

/* Site pooling.  Replaces calculate_site_proba(read_probs, n_iters, n_samples, n_processes) +
 * the mod_ratio line (m6anet/utils/inference_utils.py:53-54,74-104) for ALL flush groups of a
 * job at once, with the reference's n_processes=1 semantics: the NumPy MT19937 stream restarts
 * from `seed` at every flush group (groups follow batch_size/save_per_batch exactly as the
 * loop at inference_utils.py:33,47 forms them -- see m6a_flush_groups), sites inside a group
 * consume it sequentially, indices come from masked rejection, the 20-term product is float32
 * left-to-right, the mean over iterations is NumPy's float32 pairwise sum and one divide -- given the
 * same read probabilities the site probabilities are bit-identical to the reference's.
 *   site_prob [S] float32 out;  mod_ratio [S] float64 out = mean(read_prob >= thr)
 *   n_samples <= M6A_MAX_SAMPLES (the reference passes 20, inference_utils.py:54). */
int m6a_site_pool(m6a_ctx *ctx, const float *read_prob, const int64_t *off, int64_t n_sites,
                  int n_iters, int n_samples, float read_proba_threshold, uint32_t seed,
                  int rng_mode, int64_t batch_size, int64_t save_per_batch,
                  float *site_prob, double *mod_ratio);

/* Fused encode + pool (what run_inference does per job, inference_utils.py:14-71, minus text
 * I/O).  read_prob may be NULL when per-read output (data.indiv_proba.csv) is not wanted. */
int m6a_infer(m6a_ctx *ctx, const float *X, const uint8_t *site_kmers, const int64_t *off,
              int64_t n_sites, int n_iters, int n_samples, float read_proba_threshold,
              uint32_t seed, int rng_mode, int64_t batch_size, int64_t save_per_batch,
              float *read_prob, float *site_prob, double *mod_ratio);

/* The site probability in closed form.  The reference's estimator draws n_samples reads of a site uniformly, independently and
 * with replacement, n_iters times, and averages 1 - prod(1 - p) (m6anet/utils/inference_utils.py:74-104); what it estimates is
 *     E = 1 - (mean_i (1 - p_i)) ^ n_samples
 * and m6a_site_expectation computes E itself: no random stream, no flush groups, no seed -- the result depends on the site's
 * reads and n_samples alone, not on the kernel variant, the host-offsets hint, batch boundaries, m6a_set_job_offset or the shard.
 * The operation (tests/site_expectation_statement.py states it in NumPy float64; host and device give the same bits), for a site
 * with reads p_0 .. p_{n-1} (float32) and K = n_samples:
 *   pairs m2^K - (m1^K)^2 cancels -- one unit in the last place of a power is 1e-16 / mc_sigma in the root -- so the sums and the
 *         powers are carried as unevaluated pairs (hi, lo) of doubles and rounded once.  Every operation below is one IEEE
 *         addition, subtraction or multiplication of doubles, evaluated as written (no fma, no reassociation):
 *           two_sum(a, b):   s = a + b;  bb = s - a;  e = (a - (s - bb)) + (b - bb)               -> (s, e), a + b = s + e exactly
 *           quick(s, e):     hi = s + e;  lo = e - (hi - s)                                        -> (hi, lo)
 *           split(a):        c = 134217729.0 * a;  h = c - (c - a);  l = a - h                     -> (h, l)
 *           add_d(x, b):     (s, e) = two_sum(x.hi, b);  quick(s, e + x.lo)
 *           add(x, y):       (s, e) = two_sum(x.hi, y.hi);  quick(s, e + (x.lo + y.lo))
 *           mul(x, y):       p = x.hi * y.hi;  (ah, al) = split(x.hi);  (bh, bl) = split(y.hi);
 *                            e = ((ah * bh - p) + ah * bl + al * bh) + al * bl;  quick(p, e + (x.hi * y.lo + x.lo * y.hi))
 *   u_i   = 1.0 - (double)p_i;  w_i = u_i * u_i (one rounded product)
 *   sums  64 partial pairs a[j], b[j], j = 0..63, all (0, 0) at first; for i = 0, 1, .., n-1 in this order
 *             a[i % 64] = add_d(a[i % 64], u_i);   b[i % 64] = add_d(b[i % 64], w_i)
 *         then for h = 32, 16, 8, 4, 2, 1:  a[j] = add(a[j], a[j + h]) and b[j] = add(b[j], b[j + h]) for j < h;
 *         S1 = a[0].hi, S2 = b[0].hi
 *         (a partial that took no read is (0, 0) and add(x, (0, 0)) = x for every finite pair, while a partial that took an
 *         infinite or NaN value is NaN from that addition on; so a bag of <= 32 reads folded 16, 8, 4, 2, 1 by one lane has the
 *         bits a wavefront per site gives it: both kernel variants follow this one order)
 *   m1    = S1 / (double)n,  m2 = S2 / (double)n
 *   x^K   r = (1, 0), b = (x, 0), e = K;  while e != 0: { if (e & 1) r = mul(r, b);  e >>= 1;  if (e != 0) b = mul(b, b); };
 *         x^K = r.hi -- IEEE multiplications and additions only, no pow / exp / log
 *   site_prob = (float)(1.0 - m1^K)
 *   mc_sigma  = sqrt(max(m2^K - m1^K * m1^K, 0.0)), a double: the standard deviation of ONE iteration of the reference's
 *         estimator; mc_sigma / sqrt(n_iters) is the standard error of the number m6a_site_pool writes in its default mode
 *   mod_ratio = m6a_site_pool's: (double)count(p_i >= thr) / (double)n
 * read_prob values outside [0, 1] and NaN are not checked: they propagate through the arithmetic above (a NaN read makes the
 * site's site_prob and mc_sigma NaN and counts as below the threshold).  n_samples in 1..M6A_MAX_SAMPLES, an empty bag gives NaN
 * in all three outputs, pointers all host (synchronous) or all device (stream-ordered; m6a_set_host_offsets applies) -- the
 * rules of m6a_site_pool.  mc_sigma [S] may be NULL.  No reference counterpart: the reference has only the estimator. */
int m6a_site_expectation(m6a_ctx *ctx, const float *read_prob, const int64_t *off, int64_t n_sites, int n_samples,
                         float read_proba_threshold, float *site_prob, double *mod_ratio, double *mc_sigma);
/* What site_prob means in m6a_site_pool, m6a_infer and m6a_job_end on this context (and so in the inference a command runs from
 * an m6a_prep_sites handle).  M6A_SITE_SAMPLED (the default): the replay of the reference's random stream described at
 * m6a_site_pool.  M6A_SITE_EXPECTED: m6a_site_expectation's site_prob; n_iters, seed, rng_mode, batch_size and save_per_batch
 * (and the job offset against them) are validated as before and otherwise ignored, and no random stream, pairwise-sum plan or
 * index table is built or waited for -- m6a_create's background set-up stops at its next step when the mode is set.  mod_ratio
 * is the same in both modes.  Setting the mode back gives the default's bits again; a context on which the mode was never set
 * behaves as before.  Any other value is M6A_EINVAL and changes nothing.  m6a_last_pool_variant reports "expected-lane"
 * (every bag of the same n <= 32 reads: a lane per site) or "expected-wave" (a wavefront per site) for calls in this mode
 * and for m6a_site_expectation. */
enum { M6A_SITE_SAMPLED = 0, M6A_SITE_EXPECTED = 1 };
int m6a_set_site_mode(m6a_ctx *ctx, int mode);

/* The rank-sum test between two conditions, per site: is a site's bag of read probabilities in one set shifted against its bag in
 * another?  Two sets of sites are given as m6a_encode_reads leaves them (prob [off[n_sites]] float32 and CSR offsets off [n_sites + 1],
 * for instance the read_prob and off of two m6a_prep_sites handles); pair k compares site pair_a[k] of the first set with site
 * pair_b[k] of the second.  The test is the two-sided Mann-Whitney U test with midranks for ties, the tie-corrected variance, the
 * continuity correction and the normal approximation: scipy.stats.mannwhitneyu(a, b, use_continuity=True, alternative="two-sided",
 * method="asymptotic").  The operation (tests/ranksum_statement.py states it in NumPy; host and device give the same bits), for a
 * pair with bag a (n reads) and bag b (m reads); every comparison is the IEEE float32 comparison, so -0.0 == 0.0:
 *   gt  = #{(i, j) : a_i > b_j}                                              int64
 *   eq  = #{(i, j) : a_i == b_j}                                             int64; 2 gt + eq is twice scipy's U1
 *   tie = sum over the distinct values v of the pooled sample of t_v^3 - t_v, t_v = how often v occurs in it -- the same number is
 *         the sum over the pooled elements x of c_x^2 - 1, c_x = the pooled elements equal to x                  int64
 *   z   one double; every line is one IEEE double operation per operator, evaluated as written (no fma, no reassociation; division
 *       and sqrt round correctly on both sides):
 *           nm  = (double)n * (double)m;         N = (double)(n + m)
 *           U   = (double)(2*gt + eq) * 0.5;     d = U - nm * 0.5
 *           tc  = (double)tie / (N * (N - 1.0))
 *           var = nm / 12.0 * ((N + 1.0) - tc);  s = sqrt(var)
 *           num = max(fabs(d) - 0.5, 0.0)
 *           z   = num > 0 ? copysign(num, d) / s : copysign(0.0, d)
 *       z > 0: the reads of a score higher.  The two-sided p-value is erfc(|z| / sqrt(2)) and U / nm is the AUC (the host's business:
 *       m6anet_amd/ranksum.py).  All pooled values equal: d = 0 and z = 0, where scipy reports p = 1.
 *   undefined pairs  either bag empty, a NaN in either bag, or n + m > 2^20 (the bound keeps tie <= (n + m)^3 inside int64): gt = eq =
 *       tie = -1 and z = NaN.  Not an error.  Infinite values are ordinary values.
 * The counts are integers, so they do not depend on how they are counted; no float is added anywhere before z.  The kernel
 * (site_ranksum_kernel, a wavefront per pair) compares all pairs: about (n + m)^2 comparisons per pair, made for bags of tens to a few
 * thousand reads; the largest defined pair occupies one wavefront for about a minute.
 *   pair_a, pair_b  [n_pairs] int64, or NULL: the identity, which needs n_pairs == n_sites_a == n_sites_b (else M6A_EINVAL).  A site
 *       may appear in any number of pairs, in any order
 *   gt, eq, tie     [n_pairs] int64 out, each may be NULL;  z [n_pairs] float64 out, required
 * Pointers all host (staged, synchronous) or all device (queued on the context's stream), as stated under DATA POINTERS.  With host
 * arrays a pair index outside its set and offsets that do not start at 0 or that decrease are M6A_EINVAL before anything is queued
 * and the outputs are untouched.  With device arrays the kernel reads nothing through an index or an offset it has not checked: a
 * pair whose index is outside its set, or whose offsets are negative, decrease or exceed off[n_sites], gets the undefined pair's
 * values and raises a deferred M6A_EINVAL that the next m6a_sync returns; every other pair of the call is computed.  n_pairs == 0 is
 * M6A_OK and touches nothing.  No reference counterpart: the reference scores one condition at a time. */
int m6a_site_ranksum(m6a_ctx *ctx, const float *prob_a, const int64_t *off_a, int64_t n_sites_a,
                     const float *prob_b, const int64_t *off_b, int64_t n_sites_b,
                     const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs,
                     int64_t *gt, int64_t *eq, int64_t *tie, double *z);
/* The same test on the signal itself: m6a_site_ranksum on each of the M6A_N_FEATURES columns of two sets' X, the model-free comparison
 * beside the one on read probabilities.  X_* is [off_*[n_sites_*]][9] float32 as m6a_encode_reads takes it (for instance the X and off of
 * two m6a_prep_sites handles), so per read dwell_time, norm_std, norm_mean at position -1, then at 0, then at +1 (M6A_N_FEATURES above);
 * off_* counts rows.  A site has the same 7-mer in both sets, so its normalisation is one increasing affine map per column and ranks on X
 * are ranks on the raw signal.  For pair k and column c the result, at [k * 9 + c] of each output, is exactly m6a_site_ranksum's result
 * on two bags: column c of the rows of site pair_a[k] and column c of the rows of site pair_b[k] -- gt, eq and tie as defined above, z by
 * the lines above (one header, m6anet_amd/csrc/m6a_ranksum.h, computes it for both kernels and the host), the float32 comparisons as above.
 * tests/signal_ranksum_statement.py states it by calling the statement above per column.
 *   undefined  either bag empty or n + m > 2^20: all nine columns.  A NaN in column c of either bag: column c alone (-1, -1, -1, NaN),
 *       the other eight are computed.  Not an error.
 *   gt, eq, tie  [n_pairs][9] int64 out, row-major, each may be NULL;  z [n_pairs][9] float64 out, required
 * Pair arrays, pointers (all host: staged, synchronous, checked before anything is queued and the outputs untouched on M6A_EINVAL; or all
 * device: queued on the context's stream) and n_pairs == 0 are m6a_site_ranksum's rules.  With device arrays nothing is read through an
 * index or an offset that has not been checked: a bad pair gets the undefined values in all nine columns and raises the deferred
 * M6A_EINVAL of the next m6a_sync; every other pair is computed.  The kernel (site_signal_ranksum_kernel, a wavefront per pair) makes the
 * same (n + m)^2 comparisons per column and fetches each tile of rows once for all nine.  The nine p-values of a site are nine tests:
 * `eventalign_diff --signal` corrects them as one Benjamini-Hochberg family over every row of data.diff_signal.csv (nine per shared
 * site).  Not built: a sort-based path for very large bags, a lane-per-pair variant, effect sizes in pA (m6a_site_signal_ks below gives
 * the Kolmogorov-Smirnov statistic and the medians in X's units).
 * No reference counterpart. */
int m6a_site_signal_ranksum(m6a_ctx *ctx, const float *X_a, const int64_t *off_a, int64_t n_sites_a,
                            const float *X_b, const int64_t *off_b, int64_t n_sites_b,
                            const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs,
                            int64_t *gt, int64_t *eq, int64_t *tie, double *z);

/* The two-sample Kolmogorov-Smirnov statistic and the two medians, per pair of sites: the test that sees more than a shift of location
 * (a bag that became a mixture of two populations can keep its rank-sum near zero), and the effect size beside it.  Sets, pairs and
 * pointers are m6a_site_ranksum's.  The operation (tests/ks_statement.py states it in NumPy; host and device give the same bits), for a
 * pair with bag a (n reads) and bag b (m reads), the float32 comparisons as above (-0.0 == 0.0, infinities are ordinary values):
 *   with A(v) = #{a_i <= v} and B(v) = #{b_j <= v} for a pooled value v,
 *   d_pos = max over the pooled v of (m A(v) - n B(v))                        int64
 *   d_neg = max over the pooled v of (n B(v) - m A(v))                        int64; both >= 0 (the expression is 0 at the largest v),
 *                                                                             both <= 2^40
 *   med_a = (double)lo * 0.5 + (double)hi * 0.5 with lo = a_((n-1)/2) and hi = a_(n/2) of sorted(a), 0-based, integer division: two
 *           float32 order statistics and one line of IEEE double operations, np.median(a.astype(float64)) wherever that is finite.  A
 *           result that compares equal to zero is +0.0 (which of -0.0 and 0.0 a selection meets is not defined); +inf and -inf as the
 *           two middles give NaN, as np.median does.  med_b likewise.
 *   undefined pairs  m6a_site_ranksum's rule as it is: either bag empty, a NaN in either bag, or n + m > 2^20: d_pos = d_neg = -1 and
 *       med_a = med_b = NaN.  Not an error.
 * Derived on the host (m6anet_amd/ranksum.py): D = max(d_pos, d_neg) / (n m) in double, scipy.stats.ks_2samp's statistic; ks_sign = +1
 * where d_pos >= d_neg, else -1 (+1: a's empirical CDF lies above b's at the widest gap, so a's values tend lower); and the p-value
 * p = Q(lambda), lambda = sqrt(n m / (n + m)) D, Q the Kolmogorov limit distribution 2 sum_{k>=1} (-1)^(k-1) exp(-2 k^2 lambda^2) --
 * scipy.stats.kstwobign.sf(lambda).  That is NOT what scipy.stats.ks_2samp returns (exact for small bags, kstwo at round(en) under
 * method="asymp"); the limit is conservative for small bags (one 20 + 20 pair: 0.0047 against the exact 0.0040).  The exact
 * finite-sample p-value, ks_2samp's, is m6a_ks_exact below, from h = max(d_pos, d_neg) as it stands.
 *   d_pos, d_neg   [n_pairs] int64 out, required;  med_a, med_b [n_pairs] float64 out, each may be NULL
 * Pointers all host (staged, synchronous, checked before anything is queued and the outputs untouched on M6A_EINVAL) or all device
 * (queued on the context's stream), pair arrays and n_pairs == 0 as for m6a_site_ranksum.  With device arrays nothing is read through an
 * index or an offset that has not been checked: a bad pair gets the undefined values and raises the deferred M6A_EINVAL of the next
 * m6a_sync; every other pair is computed.  The kernel (site_ks_kernel, a wavefront per pair) makes about 1.5 (n + m)^2 comparisons per
 * pair and adds no float before the median's line.  No reference counterpart. */
int m6a_site_ks(m6a_ctx *ctx, const float *prob_a, const int64_t *off_a, int64_t n_sites_a,
                const float *prob_b, const int64_t *off_b, int64_t n_sites_b,
                const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs,
                int64_t *d_pos, int64_t *d_neg, double *med_a, double *med_b);
/* m6a_site_ks on each of the M6A_N_FEATURES columns of two sets' X [off_*[n_sites_*]][9], as m6a_site_signal_ranksum is m6a_site_ranksum
 * on them: for pair k and column c the result, at [k * 9 + c] of each output, is m6a_site_ks's result on column c of the rows of the two
 * sites (tests/ks_statement.py calls its own pair statement per column).  The medians are in the normalised units of X; their
 * conversion to pA is not built.
 *   undefined  either bag empty or n + m > 2^20: all nine columns.  A NaN in column c of either bag: column c alone, the other eight
 *       are computed.  Not an error.
 *   d_pos, d_neg  [n_pairs][9] int64 out, row-major, required;  med_a, med_b [n_pairs][9] float64 out, each may be NULL
 * Everything else is m6a_site_ks's.  The kernel (site_signal_ks_kernel, a wavefront per pair) fetches each tile of rows once for all nine
 * columns.  `eventalign_diff --signal --ks` corrects the nine p-values of a site as one Benjamini-Hochberg family over every row of
 * data.diff_signal_ks.csv.  No reference counterpart. */
int m6a_site_signal_ks(m6a_ctx *ctx, const float *X_a, const int64_t *off_a, int64_t n_sites_a,
                       const float *X_b, const int64_t *off_b, int64_t n_sites_b,
                       const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs,
                       int64_t *d_pos, int64_t *d_neg, double *med_a, double *med_b);

#define M6A_KS_EXACT_SHORT 2047                               /* min(n, m) above this: the item is undefined */
#define M6A_KS_EXACT_CELLS 100000000                          /* n m above this: the item is undefined */
/* The exact two-sided p-value of the two-sample Kolmogorov-Smirnov statistic, P(D_{n,m} >= d), per item: what
 * scipy.stats.ks_2samp(a, b, method="exact") returns, from the integers m6a_site_ks and m6a_site_signal_ks deliver -- n and m the two
 * bag sizes and h = max(d_pos, d_neg), the statistic in units of 1 / (n m), so no float comes between the counting and the p-value.
 * The operation (tests/ks_exact_statement.py states it in NumPy; host and device give the same bits), for n >= 1, m >= 1:
 *   a cell (i, j), 0 <= i <= n, 0 <= j <= m, is OUTSIDE when |m i - n j| >= h, compared in int64.  v[i][j] is the probability that a
 *   uniformly drawn monotone path from (i, j) to (n, m) meets an outside cell, (i, j) included:
 *     v[i][j] = 1.0 when (i, j) is outside;  v[n][m] = 0.0 when it is inside;  otherwise
 *     v[i][j] = ((double)(n - i) * v[i+1][j] + (double)(m - j) * v[i][j+1]) / (double)(n + m - i - j),
 *   a neighbour beyond the grid being 0.0: each product rounded on its own, then the sum, then one correctly rounded division -- no fused
 *   multiply-add, no reciprocal.  p = v[0][0].
 *   h == 0 gives 1.0 and an h above every attainable value (h > n m) gives 0.0, both by the recurrence.  Every term is positive, so
 *   nothing cancels: the relative error is about 3 (n + m) roundings down to the subnormal range (measured against exact path counts
 *   for n, m <= 12: at most 0.29 (n + m) 2^-53), and a result below the smallest subnormal is 0.0, as scipy's is.  The recurrence is
 *   symmetric under swapping the two bags, to the bit.
 *   undefined items  n < 1 or m < 1; h < 0 (the undefined pair of m6a_site_ks has d_pos = d_neg = -1); min(n, m) > M6A_KS_EXACT_SHORT
 *       (2047) or n m > M6A_KS_EXACT_CELLS (10^8, scipy's own 10 000 x 10 000): p = NaN.  Not an error.  `eventalign_diff --ks_exact`
 *       writes the limit distribution's p for such an item and says so in its p_method column.
 *   n, m, h [count] int64 in;  p [count] float64 out
 * Pointers all host (staged, synchronous) or all device (queued on the context's stream); count == 0 is M6A_OK; a null pointer, a
 * negative count or a mixture of host and device pointers is M6A_EINVAL with p untouched.  Nothing is read through n, m or h, so no
 * value of them is an error.  The kernel (ks_exact_kernel, m6anet_amd/csrc/m6a_ks_exact.hip) gives an item to a wavefront: the shorter
 * bag on j, rows i in stripes of 64 with lane l on row i0 + l one step behind lane l + 1, so that every step has all lanes on one
 * anti-diagonal; v[i][j+1] is the lane's own last result, v[i+1][j] one cross-lane move of a double, and the row between two stripes
 * (min(n, m) + 1 doubles, the reason for the first cap) stays in LDS.  Only the j at which some row of a stripe is inside the band
 * are walked.  An item costs about its inside cells plus 64 steps per stripe; the largest defined item is 10^8 divisions on one
 * wavefront.  Not built: one-sided exact p-values.  No reference counterpart. */
int m6a_ks_exact(m6a_ctx *ctx, const int64_t *n, const int64_t *m, const int64_t *h, int64_t count, double *p);

/* Streaming form of m6a_infer: the batch loop of run_inference (m6anet/utils/inference_utils.py:33-54) fed as the
 * DataLoader produces it, so a reference-side binding keeps its loader and its loop.
 *   m6a_job_begin   the arguments calculate_site_proba / the flush test get per job (inference_utils.py:47,54);
 *                   expect_sites / expect_reads size the device arrays up front (0 = unknown: they grow);
 *                   m6a_set_job_offset applies as in m6a_infer.
 *   m6a_job_feed    one batch = the arguments of m6a_encode_reads (inference_utils.py:35-37): X [r][9], site_kmers [n][3],
 *                   off [n+1] batch-local CSR offsets (off[0] = 0).  ASYNCHRONOUS: host rows are copied into a pinned
 *                   ring (the buffers are the caller's again on return), cross PCIe while earlier chunks are being
 *                   encoded, and the encoder is queued per chunk of <= ~130 k reads.  X / site_kmers may be host or
 *                   device pointers (both of a kind).  DEVICE rows are NOT copied: the encoder queued on the context's
 *                   stream reads them in place, possibly after the call has returned -- they must stay allocated and
 *                   unmodified until m6a_job_end / m6a_job_abort returns, and whatever produced them must be ordered
 *                   before the context's stream (same stream, or completed).  off is ALWAYS a host pointer -- it is
 *                   the loader's n_reads vector (data_utils.py:499).  Batches of any size, in job order.
 *   m6a_job_end     pools all sites fed so far exactly as m6a_infer would (same flush groups, same random stream) and
 *                   delivers read_prob [R] (or NULL), site_prob [S], mod_ratio [S] -- all host (synchronous) or all
 *                   device (the call still synchronises).  Closes the job, also on error.  Results are bit-identical
 *                   to one m6a_infer over the concatenated batches whenever both pick the same encoder kernel:
 *                   always when every bag has >= 16 reads (datasets are filtered to >= 20, data_utils.py:129) or when
 *                   m6a_set_encoder_variant pins it (the choice is made per chunk here, per job there; the two
 *                   kernels agree to float32 rounding); site_prob / mod_ratio are in every case exactly
 *                   m6a_site_pool of the job's read probabilities.
 *   m6a_job_size    sites / reads fed so far;  m6a_job_abort drops an open job.
 * A feed that fails voids the job: later feeds and m6a_job_end return its code.  While a job is open the other
 * compute entry points of the context return M6A_EINVAL. */
int m6a_job_begin(m6a_ctx *ctx, int n_iters, int n_samples, float read_proba_threshold, uint32_t seed, int rng_mode,
                  int64_t batch_size, int64_t save_per_batch, int64_t expect_sites, int64_t expect_reads);
int m6a_job_feed(m6a_ctx *ctx, const float *X, const uint8_t *site_kmers, const int64_t *off, int64_t n_sites);
/* The same batch in the layout the reference's loader hands its loop -- inference_collate's first three tensors
 * (m6anet/utils/data_utils.py:498-506): features f32 [r][9], kmers int64 [r][3] (every read repeats its site's three
 * vocabulary ids, :221-224), n_reads int64 [n] -- so a reference-side binding passes three data_ptr()s and converts
 * nothing.  HOST pointers only; ids outside 0..65 are M6A_EINVAL. */
int m6a_job_feed_collated(m6a_ctx *ctx, const float *features, const int64_t *kmers, const int64_t *n_reads, int64_t n_sites);
int m6a_job_size(const m6a_ctx *ctx, int64_t *n_sites, int64_t *n_reads);
int m6a_job_end(m6a_ctx *ctx, float *read_prob, float *site_prob, double *mod_ratio);
int m6a_job_abort(m6a_ctx *ctx);

/* MILModel.forward on fixed-size bags (m6anet/model/model.py:155-164 ->
 * SigmoidProdPooling.forward, pooling_blocks.py:127-129): X [B*bag][9], site_kmers [B][3],
 * site_prob[b] = 1 - prod_k (1 - p[b*bag+k]) in float32, left to right. */
int m6a_bag_forward(m6a_ctx *ctx, const float *X, const uint8_t *site_kmers, int64_t n_bags,
                    int bag, float *site_prob);

/* validate() at DataLoader num_workers=0, shuffle=False (m6anet/utils/training_utils.py:213-268):
 * n_iters passes over the sites in order; each pass draws n_samples reads of every site WITHOUT
 * replacement -- np.random.choice(n, n_samples, replace=False), m6anet/utils/data_utils.py:213-214,
 * i.e. the legacy shuffle of arange(n), the stream seeded once with `seed` -- and predicts
 * y_pred[t][s] = 1 - prod_k (1 - p[read k of the sample]) (MILModel.forward, model.py:155-164).
 * y_pred [n_iters][n_sites]; y_pred_avg [n_sites] = np.mean(y_pred, axis=0) (training_utils.py:253)
 * or NULL.  As in NumPy, the mean adds pass after pass when n_sites >= 2, and a single site takes NumPy's
 * pairwise mean of its n_iters values.  Every bag needs >= n_samples reads (NumPy raises otherwise: M6A_EINVAL).  The sampler
 * is a sequential walk over one random stream and runs on the host; gathers, products and the
 * mean run on the GPU.  m6a_validate_pool starts from read probabilities, m6a_validate encodes
 * first (read_prob [R] or NULL).  Pointers: see DATA POINTERS at the top. */
int m6a_validate_pool(m6a_ctx *ctx, const float *read_prob, const int64_t *off, int64_t n_sites,
                      int n_iters, int n_samples, uint32_t seed, float *y_pred, float *y_pred_avg);
int m6a_validate(m6a_ctx *ctx, const float *X, const uint8_t *site_kmers, const int64_t *off,
                 int64_t n_sites, int n_iters, int n_samples, uint32_t seed, float *read_prob,
                 float *y_pred, float *y_pred_avg);

/* Host-only helpers (no GPU, usable with ctx == NULL semantics: they take no ctx). */

/* Flush groups of the reference's loop (inference_utils.py:33,47): batches of `batch_size`
 * sites; batch `it` closes a group when (it+1) % save_per_batch != 0 (the reference's inverted
 * test).  Batches after the last flush -- which the reference silently never writes -- form a
 * final group here.  Writes group_off[0..G] and returns G, or M6A_EINVAL if cap < G+1. */
int64_t m6a_flush_groups(int64_t n_sites, int64_t batch_size, int64_t save_per_batch,
                         int64_t *group_off, int64_t cap);

/* Sites the REFERENCE writes for this geometry: everything up to its last flush.  Batches after it are computed
 * by nobody and never reach the CSVs there (an even batch count always loses the last batch at the default
 * save_per_batch = 2); the reference-compatible CLI mode (--drop_unflushed_tail) cuts its output here. */
int64_t m6a_reference_written_sites(int64_t n_sites, int64_t batch_size, int64_t save_per_batch);

/* Contiguous, flush-group-aligned site shards balanced by read count for n_shards GPUs
 * (sites are independent; aligning to groups keeps results independent of the GPU count).
 * off is a HOST pointer.  Writes shard_site_off[0..n_shards]. */
int m6a_shard_plan(const int64_t *off, int64_t n_sites, int64_t batch_size, int64_t save_per_batch,
                   int n_shards, int64_t *shard_site_off);

/* The job's one exchange: every rank's site_prob / mod_ratio to rank `dst` over RCCL
 * (xGMI inside a node) -- the counterpart of nothing in the reference, which has no multi-device path; it is what
 * a launcher calls after each rank ran m6a_infer on its shard (m6a_shard_plan, m6a_set_job_offset).
 *   m6a_comm_unique_id   rank 0 makes the 128-byte RCCL id (ncclGetUniqueId); the launcher hands it to every rank
 *                        by whatever transport it has (its process group, MPI, a file);
 *   m6a_comm_init        ncclCommInitRank on the context's device -- one communicator per context;
 *   m6a_gather           shard_site_off [world+1] (always a HOST array) are the cuts of m6a_shard_plan;
 *                        site_prob / mod_ratio hold this rank's shard_site_off[rank+1] - shard_site_off[rank] sites;
 *                        site_all / mod_all [shard_site_off[world]] are written on rank dst only (may be NULL
 *                        elsewhere).  ONE grouped send/recv exchange on the context's stream, ragged shards land at
 *                        their offsets without padding.  Data pointers all device (stream-ordered, the caller
 *                        synchronises with m6a_sync) or all host (staged through the context, synchronous): DATA POINTERS at the top;
 *   m6a_gather_reads     the same exchange for the per-read output (data.indiv_proba.csv needs it on the rank that
 *                        writes): read_prob holds this rank's shard_read_off[rank+1] - shard_read_off[rank] reads
 *                        (shard_read_off[r] = off[shard_site_off[r]] of the job's CSR offsets), read_all on dst;
 * RCCL is bound at run time (dlopen of librccl; M6A_RCCL_LIB names a specific copy): a process that never calls
 * these needs no RCCL.  M6A_EUNSUPPORTED if the library cannot be found. */
#define M6A_COMM_ID_BYTES 128
int m6a_comm_unique_id(void *id_out);
int m6a_comm_init(m6a_ctx *ctx, const void *unique_id, int rank, int world_size);
int m6a_gather(m6a_ctx *ctx, const float *site_prob, const double *mod_ratio, const int64_t *shard_site_off,
               int dst, float *site_all, double *mod_all);
int m6a_gather_reads(m6a_ctx *ctx, const float *read_prob, const int64_t *shard_read_off, int dst, float *read_all);
int m6a_comm_destroy(m6a_ctx *ctx);
/* What the communicator ITSELF reports, for a launcher or a benchmark line that has to certify an N-rank run instead of
 * trusting its own arguments: m6a_comm_count = ncclCommCount (the ranks RCCL formed the communicator with);
 * m6a_comm_info = ncclCommUserRank, ncclCommCuDevice (the HIP device the communicator is bound to) and ncclGetVersion
 * (e.g. 22707); any of the three pointers may be NULL.  m6a_device_link = how two visible HIP devices are connected:
 * link_type as hipExtGetLinkTypeAndHopCount reports it (hsa_amd_link_info_type_t: 2 = PCIe, 4 = xGMI), hop count,
 * and whether dev_a can map dev_b's memory (hipDeviceCanAccessPeer) -- what decides whether the gather's direct
 * send/recv writes travel over xGMI.  No reference counterpart (it has no multi-device path). */
int m6a_comm_count(m6a_ctx *ctx, int *ranks_seen);
int m6a_comm_info(m6a_ctx *ctx, int *rank, int *device, int *rccl_version);
int m6a_device_link(int dev_a, int dev_b, int *link_type, int *hops, int *peer_access);
/* HIP devices visible to this process (0 if none / no runtime): what a launcher sizes `world` against. */
int m6a_device_count(void);

/* The random stream the site sampling replays, by itself: the first n_words 32-bit outputs of NumPy's legacy generator
 * after np.random.seed(seed) (m6anet/scripts/inference.py:86) -- MT19937 seeded by init_genrand, the words
 * RandomState.bytes / randint consume (m6anet/utils/inference_utils.py:85 draws from it through np.random.choice).
 * Generated on the GPU in up to 32 parallel segments (GF(2) jump-ahead).  words: host or device pointer; a device-pointer
 * call is stream-ordered (m6a_sync).  Known-answer vectors: tests/golden/mt19937_seed*_first4096.u32. */
int m6a_random_stream(m6a_ctx *ctx, uint32_t seed, int64_t n_words, uint32_t *words);

/* Per-kernel timing with HIP events on the context's stream (bench.py's live roofline).
 * kind: 0 = read encoder, 1 = site pooling.  on: 0 off, 1 both kinds, 2 the encoder only, 3 the pooling only (two events per
 * timed launch cost ~5 us each on the stream).  m6a_profile_read synchronises the stream. */
int m6a_profile_enable(m6a_ctx *ctx, int on);
int m6a_profile_read(m6a_ctx *ctx, int kind, double *total_ms, int64_t *n_launches);
/* The shader clock the LAST profiled launch of `kind` ran at, from inside the kernel: while profiling is on, lane 0 of up to
 * 64 workgroups spread over the grid (and over the 8 XCDs) stamps s_memtime (shader cycles) and s_memrealtime (constant
 * 100 MHz) at its start and end; GHz = cycles / real time of each such wave.  bench.py prices the rooflines at this clock
 * beside the nominal 2.4 GHz (a kernel that makes the part clock down is not an issue-limited kernel).  span_ms = first start
 * to last end among the stamped waves (a cross-check of the HIP-event duration).  Any out pointer may be NULL; n_waves = 0
 * when nothing was stamped (no profiled launch yet; kernels without stamps: the scan and LDS-table pooling fallbacks).
 * Launches outside profiling carry a null stamp pointer. */
int m6a_profile_clock(m6a_ctx *ctx, int kind, double *ghz_median, double *ghz_min, double *ghz_max, double *span_ms, int *n_waves);
/* Which read-encoder kernel runs.  0 = auto (default) = the REFERENCE'S BITS on every input: the 16-slot kernels perform the
 * reference's float32 operations in the reference's order all the way (layer sums as fma chains over k then the bias, batch
 * norm as one fma, the 32 -> 1 layer in the capture machine's sgemv order, Sleef's expf: blocks.py:249-254, pooling_blocks.py:52
 * as torch executes them on an AVX-512 host) -- enc_site16_kernel when every bag has >= 16 reads and the job fits 32-bit
 * indices, enc_kernel otherwise; same operations, same bits.  This is what the CLI (`--encoder reference`, its default),
 * INTEGRATION.md's stub, bench.py's headline and every caller that sets nothing get: ONE kernel family for the product and
 * the quoted number.
 *   1 = the same, said explicitly;   3 = the 16-slot arithmetic behind enc_kernel's per-lane walk even where the scalar site
 *   chain would do (A/B and tests);
 *   2 = the 12-slot kernel, strictly (every bag must have >= 16 reads: a call that violates this reports M6A_EINVAL at the
 *   next sync);   4 = "fast": the 12-slot kernel where every bag has >= 16 reads, the 16-slot kernels elsewhere.
 * The 12-slot kernel (enc_csite_kernel) is OPT-IN: it issues 106 MFMAs per 32-read tile instead of 116 (2.03 vs 2.16 ms per
 * 20 M reads, 4-5 % per step) by adding a site's six embedding terms and b1 pre-summed and summing the 32 -> 1 layer in
 * register order -- two departures from the reference's order.  Its read probabilities are within the reference test's
 * rtol 1e-5 / atol 1e-8 (m6anet/tests/test_inference.py:32) on every fixture and on 218 M reads of the full-size configs; a
 * random fuzz finds a few reads in 10^10 beyond that bar -- 4 of 20 G at up to 1.005 x in round 5, none of 20 G and 4 of 14 G at up to
 * 1.08 x in round 6 -- all far inside north_star's absolute 1e-5.
 * The environment variable M6A_ENCODER=auto|reference|general16|csite12|walk16|fast preselects 0 / 0 / 1 / 2 / 3 / 4 in every
 * context the process creates; any other value makes m6a_create fail with M6A_EINVAL. */
int m6a_set_encoder_variant(m6a_ctx *ctx, int mode);
const char *m6a_last_encoder_variant(const m6a_ctx *ctx);   /* "general16" (auto, 1, 3) | "csite12" (2, 4 where it applies) */
/* The __global__ function the last encode launched: "enc_site16_kernel" (16 slots, scalar 32-bit site chain: every bag
 * >= 16 reads), "enc_kernel" (16 slots, per-lane 64-bit walk: any bags; mode 3 forces it), "enc_csite_kernel" (12 slots).
 * The two 16-slot kernels perform the same float32 operations: same bits. */
const char *m6a_last_encoder_kernel(const m6a_ctx *ctx);
/* Tuning knob for ragged bags: 0 = auto (default: per-bag-size index tables once the work seen pays for them, else
 * the stream-replaying scan kernels, their driver chosen by the parallelism on offer), 1 = scan, one wavefront per
 * flush group, 2 = scan, counting pass + one wavefront per site, 3 = index tables always (M6A_EUNSUPPORTED if a bag
 * exceeds 4096 reads).  Results are identical. */
int m6a_set_scan_driver(m6a_ctx *ctx, int mode);
/* Tuning knob for uniform bags (n <= 32, n_samples = 20): 0 = auto (default: the register kernel
 * where it applies), 1 = LDS-gather kernel, 2 = register kernel (bags in VGPRs, draws through the
 * VGPR index mode).  Results are identical. */
int m6a_set_table_variant(m6a_ctx *ctx, int mode);
/* pooling kernel variant used by the last pool/infer call:
 * "table-reg" | "table" (uniform bags) | "ragged-table" | "scan-group" | "scan-site" (ragged bags) |
 * "expected-lane" | "expected-wave" (M6A_SITE_EXPECTED and m6a_site_expectation) */
const char *m6a_last_pool_variant(const m6a_ctx *ctx);

const char *m6a_version(void);

/* `dataprep --device gpu` (m6anet/scripts/dataprep.py:54-70; include/m6a_io.h for the host half).  Streams eventalign.txt into HBM
 * on device device_id and computes what m6a_io_dataprep_rows computes on the host: the index runs (or, with index_path non-NULL,
 * the rows of that eventalign.index) and every run's candidate rows, as an m6a_io_prep_table that m6a_io_dataprep_write turns
 * into eventalign.index, data.json, data.info and data.log, byte-identical to m6a_io_dataprep.  Needs no weights and no ctx.
 * The whole file stays resident: device memory is capped at free memory minus a margin (M6A_PREP_BUDGET_MB lowers it), and a file
 * that does not fit is M6A_ENOMEM, with text that names --device cpu.  M6A_PREP_WINDOW_KB > 0 parses the file in windows of that
 * size instead (the cut rule is stated at m6a_prep_sites_build_windows; the front half is shared) and the table is the same; it
 * is ignored when index_path is given, because the rows of an index are arbitrary byte ranges.  M6A_PREP_CHUNK_KB (default 65536, rounded up to 4 KB)
 * sets the size of the pinned upload chunks.  Runs the device declines (numbers outside the fast paths, events out of key order,
 * malformed lines) are marked M6A_PREP_RUN_HOST; the writer combines them on the host.  Errors: M6A_EFORMAT for a file without a
 * header line or a line with fewer than three tabs (the host's M6A_IO_EFORMAT), M6A_EIO for a missing file or index; the text is
 * in m6a_prep_last_error() (thread-local). */
typedef struct m6a_prep m6a_prep;
struct m6a_io_prep_table;
int m6a_prep_eventalign(int device_id, const char *path, int n_neighbors, const char *index_path, m6a_prep **out);
const struct m6a_io_prep_table *m6a_prep_table(const m6a_prep *p);    /* owned by p */
/* milliseconds of the phases: [0] upload + newline count, [1] newline offsets, [2] lines, runs, combine and windows, [3] results to
 * the host, [4] the host's run table; [5] = the upload's rate in GB/s (file bytes / [0]) */
int m6a_prep_times(const m6a_prep *p, double *ms6);
void m6a_prep_free(m6a_prep *p);
const char *m6a_prep_last_error(void);

/* `eventalign_inference`: eventalign.txt -> the arrays m6a_io_load_sites makes of `dataprep` + data.json (n_neighbors = 1, no
 * --compress), without the JSON and with X left in HBM for m6a_infer.  The front half is m6a_prep_eventalign's; the back half does on
 * the device what m6a_io_dataprep_write and then the loader do with its candidate rows: per transcript (ids in order of first
 * appearance) its runs in file order, counting stopped after readcount_max + 1 runs, transcripts with fewer than readcount_min runs
 * dropped, a read index seen again keeping its first place and taking the later run's rows; rows sorted by (transcript, position,
 * place); reads of one site must agree on the 7-mer; a site is kept with >= min_segment_count and >= 20 reads (DEFAULT_MIN_READS);
 * X = (float)((v - mean) / std) in f64 with the norm table in m6a_io_load_sites' form (n_norm = 0: no normalisation).  The arrays
 * equal m6a_io_load_sites' on the two-step output, X bit for bit.  Runs the front half declines go to `host` (m6a_io_runs_rows,
 * m6a_io_rows_table, m6a_io_rows_free, m6a_io_last_error of libm6a_io.so), and their rows join the device's before the runs are
 * selected; a failure there is returned with the host half's own text (`error` may be NULL).
 * Only ids come back: per segment of equal contig bytes 24 B and its name, per site off / transcript / position / 7-mer, per read
 * its read id; d2h_bytes counts every device-to-host byte of the call (m6a_prep_sites_fetch adds its own).  X, site_kmers and off
 * are device pointers owned by the handle; so are read_prob [R], site_prob [S] and mod_ratio [S], the outputs to give m6a_infer
 * (after m6a_set_host_offsets(off_host)), which m6a_prep_sites_fetch copies to host memory.  Errors as m6a_prep_eventalign's, plus
 * M6A_EFORMAT with the host's text for disagreeing 7-mers, a missing 5-mer in the norm table or a site outside the vocabulary; a
 * job over the device budget is M6A_ENOMEM and its text names the two-step path.  ms: [0] upload, [1] newline offsets, [2] lines,
 * runs, combine and windows, [3] back half on the device (its small copies of segments and per-site arrays included), [4] host
 * (names, declined runs), [5] the copy of the read ids (m6a_prep_sites_fetch adds the time of its own copies), [6] the upload's GB/s,
 * [7] the whole call.
 *
 * m6a_prep_sites_build_multi: several files are replicates, pooled as m6a_io_load_sites pools several input directories, and the
 * arrays equal the loader's on `dataprep` of every file (same readcount_min / readcount_max / min_segment_count) -- X bit for bit.
 * Every file goes through both halves on its own, without the 20-read floor and without the per-site checks; its text, line records
 * and candidate rows are released before the next file is uploaded, and what stays is X and the read id of the reads of its sites
 * with >= min_segment_count reads.  Sites are keyed by (transcript name, position); the pooled sites are the union in order of first
 * appearance (file 0's in file 0's order, then what file 1 adds, ...), a site's reads are its parts in file order, and it is kept
 * when the SUM of its reads is >= 20.  Kept sites only are checked, lowest first: the normalisation factors of the first part's
 * 7-mer, then every later part's 7-mer against it ("replicates disagree on the sequence of <tx>:<pos>"), then the vocabulary.
 * read_rep [R] is the position of each read's file in `paths` (a file without sites still takes its number), filled on the host from
 * the 4 n_paths bytes per kept site that come back; nothing comes back per dropped site, and per read only its id.  tx_blob /
 * tx_off name the transcripts of all files in order of first appearance.  ms sums the files' phases; the union and the pooled copy
 * are counted in [3].  m6a_prep_sites_build is the n_paths = 1 case (n_rep = 1, read_rep all 0).  peak_bytes is the high-water mark
 * of the call's device allocations, the handle's own arrays included.
 *
 * m6a_prep_sites_build_windows: m6a_prep_sites_build_multi with a window size.  window_bytes = 0 keeps every file resident while it
 * is parsed (about 3 bytes of device memory per byte of text at the peak); < 0 takes M6A_PREP_WINDOW_KB from the environment (unset or
 * 0: resident), which is what the two entry points without the argument do.  W = window_bytes > 0, rounded up to a multiple of
 * 4096, parses each file as consecutive windows, and the arrays are the same bit for bit:
 *   range    window k is file bytes [b_k, e_k), b_0 = 0; e_k is the byte after the last '\n' among the W bytes from b_k, or the
 *            file's end n when b_k + W >= n.  Only that last window may end without a newline, and in every other one the read
 *            index is atoll of the text up to e_k.  Line 0 of window 0 is the header; later windows have none.
 *   cut      runs are formed over the window's lines as over a file's.  When e_k < n the last run may go on behind e_k: it is not
 *            of this window, and b_{k+1} is its first byte; a window without a line that has a tab gives b_{k+1} = e_k.  A window
 *            whose only run starts at b_k, or that holds no newline, is done again with 2 W, 4 W, ... bytes from b_k until a second
 *            run starts in it or it reaches n.  Lines without a tab between two runs belong to neither.
 *   errors   "no header line" is window 0's; "short line at byte" names the file offset whole-file mode names, since windows go in
 *            order and the first that holds such a line ends the call.
 *   across   the first run of a window starts a segment; both halves intern contig names by their bytes, so a contig cut by a
 *            window is one transcript and the ranks of its runs go on.
 * What stays on the device while the windows pass is two windows of text, the scratch of one, and the runs (72 B each) and
 * candidate rows found so far; the budget is checked against that, not against the file's size, and the back half still needs the
 * rows of the whole file at once.  Per window only totals come back (counts, the last newline, the dropped run's start).
 * n_windows is the number of windows summed over the files (1 per resident file) and window_bytes the largest window used,
 * growth included (0 when every file was resident).  ms[0] is then the time the call waited for uploads, most of which run under
 * the previous window's kernels, and ms[6] the copy thread's own rate. */
typedef struct m6a_prep_sites m6a_prep_sites;
struct m6a_io_rows;
typedef struct m6a_prep_host_half {
    int (*rows)(const char *eventalign_path, int64_t n_runs, const int64_t *start, const int64_t *end, const int64_t *read,
                int n_neighbors, int n_threads, struct m6a_io_rows **out);
    const struct m6a_io_prep_table *(*table)(const struct m6a_io_rows *r);
    void (*free)(struct m6a_io_rows *r);
    const char *(*error)(void);
} m6a_prep_host_half;
typedef struct m6a_prep_sites_info {
    int64_t n_sites, n_reads, n_tx;
    const float *X;                 /* device [R][9] */
    const uint8_t *site_kmers;      /* device [S][3] vocabulary ids */
    const int64_t *off;             /* device [S+1] */
    float *read_prob, *site_prob;   /* device [R], [S]: m6a_infer's outputs */
    double *mod_ratio;              /* device [S] */
    const int64_t *off_host;        /* [S+1] */
    const uint32_t *site_tx;        /* [S] transcript of each site: tx_blob[tx_off[t], tx_off[t + 1]) */
    const int64_t *site_pos;        /* [S] */
    const char *site_kmer7;         /* [S][7], no terminators */
    const char *tx_blob;
    const int64_t *tx_off;          /* [n_tx + 1] */
    const double *read_ids;         /* [R] */
    double ms[8];
    int64_t d2h_bytes;
    int n_rep;                      /* files pooled */
    const int32_t *read_rep;        /* [R] replicate of each read */
    int64_t peak_bytes;
    int64_t n_windows, window_bytes;
    int64_t n_bgzf_blocks, compressed_bytes;    /* BGZF inputs (below): blocks and file bytes, summed over the files; 0 for plain text */
    double ms_inflate;                          /* their inflate and CRC kernels and the newline count over the inflated text */
    int64_t n_declined_sites;                   /* m6a_json_sites_build (below): sites that went through the host half; else 0 */
} m6a_prep_sites_info;
int m6a_prep_sites_build(int device_id, const char *path, int readcount_min, int readcount_max, int min_segment_count,
                         const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm,
                         const m6a_prep_host_half *host, int n_threads, m6a_prep_sites **out);
int m6a_prep_sites_build_multi(int device_id, const char *const *paths, int n_paths, int readcount_min, int readcount_max,
                               int min_segment_count, const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm,
                               const m6a_prep_host_half *host, int n_threads, m6a_prep_sites **out);
int m6a_prep_sites_build_windows(int device_id, const char *const *paths, int n_paths, int readcount_min, int readcount_max,
                                 int min_segment_count, const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm,
                                 const m6a_prep_host_half *host, int n_threads, int64_t window_bytes, m6a_prep_sites **out);
/* Read names (`eventalign_inference --read_names`): nanopolish and f5c run with --print-read-names write the read's UUID into field
 * 4 where the integer read_index stands otherwise.  m6a_prep_sites_build_names is m6a_prep_sites_build_windows with one more
 * argument; read_names = 0 is that call exactly.  With read_names != 0:
 *   format   a read name is exactly 36 bytes, 8-4-4-4-12 lowercase hex digits with '-' at offsets 8, 13, 18 and 23 (128 bits; it
 *            prints back as the same bytes).  Every body line with at least three tabs carries one in field 4.
 *   twin     the twin of a named file is the same file with each name replaced by its dense index 0, 1, ... in order of first
 *            appearance over those lines, in plain digits.  The call gives what it gives on the twin: every array of the handle is
 *            equal, X bit for bit, and read_ids holds the indices.  A run starts where the contig bytes or the 128-bit name change;
 *            the names are kept beside the runs (16 B per line while a window is resident, 16 B per run after it, counted against
 *            the budget) and interned on the device after a file's last window -- a stable radix sort of the run numbers by name,
 *            group heads, the groups ranked by their first run -- before anything reads a run's read index.  The duplicate rule,
 *            the host half and the pooling of replicates see integers.
 *   table    m6a_prep_sites_read_names: names16 [name_off[n_rep]][16], the names' 16 bytes (the 32 hex digits, first digit first);
 *            file f's names in index order are rows [name_off[f], name_off[f + 1]); every file has a table of its own.  Owned by
 *            the handle; n_rep = 0 and null pointers for a handle built without names.  One copy of 16 bytes per distinct name
 *            comes to the host per file and is counted in d2h_bytes -- that is all the names add to it; the table also stays on
 *            the device, where m6a_prep_sites_write_csv and both _bgzf forms print <uuid> (one file) or <uuid>_<replicate> in the
 *            read-id column of data.indiv_proba.csv, the twin's other bytes unchanged.
 *   errors   anything else in field 4 -- upper case, 35 or 37 bytes, a misplaced dash, a plain integer, nothing -- is M6A_EFORMAT
 *            "<path>: read name at byte <file offset of the field>: not a lowercase UUID".  Of all format errors of the file, "short
 *            line at byte" included, the one at the lowest file offset is reported, in windows too.
 * BGZF input needs nothing of its own (the inflated text is the text).  m6a_prep_sites_intern_ms: the time of the interning, also
 * part of ms[3]. */
int m6a_prep_sites_build_names(int device_id, const char *const *paths, int n_paths, int readcount_min, int readcount_max,
                               int min_segment_count, const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm,
                               const m6a_prep_host_half *host, int n_threads, int64_t window_bytes, int read_names, m6a_prep_sites **out);
int m6a_prep_sites_read_names(const m6a_prep_sites *p, const uint8_t **names16, const int64_t **name_off, int *n_rep);
double m6a_prep_sites_intern_ms(const m6a_prep_sites *p);
/* Streams (`eventalign_inference --eventalign -`, a FIFO, /dev/fd/N): in all four entry points above a path `-` is file descriptor 0,
 * and any path that fstat shows is not a regular file is a stream -- text that comes once and in order, of a length known when it
 * ends.  A regular file takes the paths above untouched.  Replicates may mix files and streams, each parsed on its own, in order;
 * `-` given twice is M6A_EINVAL before anything is opened.
 *   windows  a stream is always parsed in windows: window_bytes > 0 or M6A_PREP_WINDOW_KB as for files, and with neither set
 *            M6A_PREP_STREAM_WINDOW_BYTES (256 MB).  With `data` all the bytes the stream delivered, the windows are those of a
 *            regular file that holds `data`, at the same size: window k is the `size` bytes from b_k and the last one exactly when no
 *            byte follows them (the file rule b_k + size >= n), cut and growth as stated above.  So every array of the handle, X
 *            bit for bit, n_windows, window_bytes and every error's code, text and byte offset are the file's, however the writer
 *            cut its writes.  In error texts the path is the one given (`-`).
 *   device   two windows of text, the scratch of one, and the kept runs and rows, as for files: a stream of any length goes through
 *            as long as what is kept fits.  The bytes a window shares with the next (the dropped run, what follows the last newline)
 *            are copied on the device and cross the link once; the kept arrays grow geometrically, since no length projects them.
 *   saved    the back half cannot read a stream again, so every window saves, while its text is resident, the contig bytes of each
 *            run that can head a segment and the bytes of each declined run, in two device arrays that count against the budget and
 *            in peak_bytes; what comes back from them (the segment names; the declined runs the host half is given, through a
 *            temporary file m6a_declined_XXXXXX in TMPDIR, removed before the call returns) counts in d2h_bytes.  Over the budget
 *            is M6A_ENOMEM with text that names a smaller --window_mb.
 *   refused  a stream that starts 1f 8b: M6A_EINVAL, compressed input from a stream is not implemented (the text names
 *            `bgzip -dc FILE |`); m6a_prep_eventalign on a stream, with or without index_path: M6A_EINVAL, since the index and the
 *            writer read the file again.  A failing read() is M6A_EIO "cannot read <path>".
 * m6a_prep_sites_stream_bytes: the bytes read from streams, summed over the files; m6a_prep_sites_n_streams: how many of the files
 * were streams.  Both are 0 for a handle built from regular files. */
#define M6A_PREP_STREAM_WINDOW_BYTES ((int64_t)256 << 20)
int64_t m6a_prep_sites_stream_bytes(const m6a_prep_sites *p);
int64_t m6a_prep_sites_n_streams(const m6a_prep_sites *p);
const m6a_prep_sites_info *m6a_prep_sites_get(const m6a_prep_sites *p);     /* owned by p */
int m6a_prep_sites_fetch(m6a_prep_sites *p, float *read_prob, float *site_prob, double *mod_ratio);
/* host copies of X [R][9], site_kmers [S][3] and off [S+1], for inspection (counted in d2h_bytes like every other copy) */
int m6a_prep_sites_inputs(m6a_prep_sites *p, float *X, uint8_t *site_kmers, int64_t *off);
void m6a_prep_sites_free(m6a_prep_sites *p);

/* Grouped input (`eventalign_inference --grouped`): nanopolish and f5c walk a coordinate-sorted BAM, so every transcript's lines come
 * in one stretch, and every rule of the back half is per transcript.  m6a_prep_group delivers the sites of one file in batches, as
 * transcripts complete, and what it keeps on the device follows the window and the group size, not the file.
 *   grouped  Take the file's runs in file order, as m6a_prep_sites_build forms them (lines without a tab belong to no run).  The
 *            input is grouped when no contig name heads a run after a run with a different contig has followed an earlier run of that
 *            name.  Otherwise the offender is the first run in file order that breaks the rule, and the call that meets it returns
 *            M6A_EFORMAT "<path>: transcript <name> appears again at byte <start of that run> after other transcripts: the input is
 *            not grouped by transcript (run without --grouped)" -- the same at every window size and group size, a reappearance
 *            inside one batch included: the host sees every segment's name and keeps the set of closed names.
 *            tests/grouped_statement.py states the rule in plain Python.
 *   promise  On grouped input the batches' arrays, one after the other, are m6a_prep_sites_build's on the same file, X bit for bit
 *            (every batch numbers its transcripts itself: compare by name).  On any other input the error above; never other rows.
 *   windows  The text is always parsed in windows: window_bytes > 0, else M6A_PREP_WINDOW_KB, else M6A_PREP_STREAM_WINDOW_BYTES, for
 *            regular files too; a file, `-`, a FIFO.  BGZF content is M6A_EINVAL (windows over compressed input).
 *   batches  After each window the kept runs in front of the last contig stretch -- the maximal tail of segments with one name,
 *            compared by name since segments break at window edges -- are closed.  When the runs and rows of the closed part reach
 *            group_bytes (<= 0: M6A_PREP_GROUP_KB, default M6A_PREP_GROUP_KB_DEFAULT; profiles/r30_grouped_input.json), or the input
 *            ends, the back half's stages run on the closed part alone (declined runs through `host` as ever), and the closed runs and
 *            rows leave the kept arrays.
 *   flush    Every delivered batch but the last ends on a boundary m6a_flush_groups(n, batch_size, save_per_batch, ...) gives for a
 *            longer job (the boundaries depend on the batch index alone), so m6a_set_job_offset(first_site) holds for every batch.
 *            The sites behind the last such boundary -- fewer than one flush group -- stay on the device and head the next batch.  A
 *            batch with no deliverable site is not delivered; parsing goes on.
 *   errors   With one defect in the file, the code and text are m6a_prep_sites_build's.  With several, the one met first in batch
 *            order is reported: a window's format error before the batch its runs would have joined, a batch's site error before
 *            anything of a later window.  After an error every later call repeats it.
 * m6a_prep_group_next: *batch is an ordinary m6a_prep_sites handle (m6a_prep_sites_get, _fetch, _inputs, the CSV writers and _free
 * work on it as they are), NULL at the end.  Only one batch may be alive at a time: asking for the next with a live batch is
 * M6A_EINVAL.  m6a_prep_group_info: n_sites, n_reads and first_site are the last batch's (first_site = the sites of all batches
 * before it); max_kept_runs / max_kept_rows the high-water marks of the kept arrays; total_runs / total_rows what the back halves
 * have taken so far; peak_bytes, d2h_bytes, n_windows, window_bytes, stream_bytes as m6a_prep_sites_info's, over the whole group. */
#define M6A_PREP_GROUP_KB_DEFAULT ((int64_t)262144)
typedef struct m6a_prep_group m6a_prep_group;
typedef struct m6a_prep_group_counts {
    int64_t n_batches, n_sites, n_reads, first_site;
    int64_t max_kept_runs, max_kept_rows, total_runs, total_rows;
    int64_t peak_bytes, d2h_bytes, n_windows, window_bytes, stream_bytes, group_bytes;
} m6a_prep_group_counts;
int m6a_prep_group_open(int device_id, const char *path, int readcount_min, int readcount_max, int min_segment_count,
                        const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm,
                        const m6a_prep_host_half *host, int n_threads, int64_t window_bytes, int64_t group_bytes, int64_t batch_size,
                        int64_t save_per_batch, m6a_prep_group **out);
int m6a_prep_group_next(m6a_prep_group *g, m6a_prep_sites **batch);
int m6a_prep_group_info(const m6a_prep_group *g, m6a_prep_group_counts *counts);
void m6a_prep_group_close(m6a_prep_group *g);

/* `inference --loader device`: one directory of data.info + data.json -> the handle m6a_prep_sites_build returns, with the arrays
 * m6a_io_load_sites makes of that directory (include/m6a_io.h) -- X bit for bit -- and X, site_kmers and off left in HBM for m6a_infer.
 * Format: data.info is the loader's (a header line, then <transcript>,<position>,<start>,<end>,<n_reads>; rows with fewer than
 * min_reads reads are dropped, the others are the sites, in file order); bytes [start, end) of data.json hold the site's record
 *   {"<transcript>":{"<position>":{"<7-mer>":[[n, n, n, n, n, n, n, n, n, n], ...]}}}
 * with ' ', '\n', '\r', '\t' allowed between tokens: nine features and the read id per row.  X = (float)((v - mean) / std) in f64 with
 * the three 5-mers' factors (the norm table in m6a_io_load_sites' form), (float)v with n_norm = 0.
 * Accepted tokens: an optional '-', digits with at most one '.', at least one digit, no exponent, at most 19 significant digits
 * and at most 27 digits behind the point; they are converted exactly (the bits of strtod and of Python's float(); the method is
 * stated in m6anet_amd/csrc/m6a_json.h).
 * Decline rule: a site is REGULAR when its range lies in the file and is below 2 GB, the record follows the grammar with nothing
 * but whitespace behind it, the first key is the row's transcript and the second the decimal of its position, there is one
 * sequence key of 7 bytes without a backslash, every row holds exactly ten accepted tokens, there are n_reads rows, and the three
 * 5-mers are in the norm table (n_norm > 0) and in the 66-word vocabulary.  The kernels fill the rows of regular sites.  Every other
 * site is DECLINED -- never failed by the device -- and goes, in ascending order, through `host` (m6a_io_info_open, m6a_io_info_get,
 * m6a_io_info_rows, m6a_io_info_free, m6a_io_last_error of libm6a_io.so), which runs the loader's own per-site body.
 * Error rule: a declined site the loader parses (one with 1e-05 or NaN in it) has its rows copied to their place; the first one it
 * does not parse ends the call with the loader's code (as M6A_EFORMAT / M6A_EIO) and text, which is what m6a_io_load_sites reports
 * for the directory.  data.info's own errors and "no site with at least <min_reads> reads" are the loader's too.
 * Refused with M6A_EINVAL before anything is opened or allocated: n_dirs > 1 (replicates stay with the host loader) and a *.m6astore
 * path.  data.json goes up whole through the pinned chunk pair (M6A_PREP_CHUNK_KB) under the budget (M6A_PREP_BUDGET_MB, or free
 * memory less a margin), together with everything the handle keeps; over it the call is M6A_ENOMEM and its text names --loader host.
 * One status byte per site and the read ids come back, nothing else per read; the 7-mers the host needs for the CSV rows it reads
 * from the pinned chunks on their way up.  Every field of m6a_prep_sites_info is filled (n_rep = 1, n_windows = 1, the BGZF fields
 * 0, n_declined_sites), so m6a_prep_sites_fetch, _inputs and the CSV writers work on the handle.  ms: [0] upload, [3] kernels, [4]
 * host (data.info, declined sites), [5] the copy of the read ids, [6] the upload's GB/s, [7] the whole call; [1] and [2] are 0. */
struct m6a_io_info;
struct m6a_io_info_table;
typedef struct m6a_json_host_half {
    int (*open)(const char *dir, int min_reads, struct m6a_io_info **out);
    const struct m6a_io_info_table *(*table)(const struct m6a_io_info *info);
    int (*rows)(struct m6a_io_info *info, const int64_t *sites, int64_t n, const char *norm_kmers, const double *norm_mean,
                const double *norm_std, int n_norm, int n_threads, float *X, double *read_ids, uint8_t *site_kmers, char *kmer7);
    void (*free)(struct m6a_io_info *info);
    const char *(*error)(void);
} m6a_json_host_half;
int m6a_json_sites_build(int device_id, const char *const *dirs, int n_dirs, int min_reads, const char *norm_kmers,
                         const double *norm_mean, const double *norm_std, int n_norm, const m6a_json_host_half *host, int n_threads,
                         m6a_prep_sites **out);

/* `compute_norm_factors`: the per-5-mer mean and std of the nine features that `train` and `inference` normalise with, from the
 * Train rows of data.info.labelled and data.json.  The operation, on this route and on m6a_io_norm_factors (include/m6a_io.h), whose
 * bits this one returns; tests/norm_statement.py states it in plain Python:
 *   sites     n_sites rows in the caller's order (the Train rows in file order; no read-count filter; a row given twice counts twice):
 *             transcript tx_blob[tx_off[i], tx_off[i + 1]), pos[i], bytes [start[i], end[i]) of json_path -- one record in the format
 *             stated at m6a_json_sites_build -- and n_reads[i].  Every number is the double Python's float() gives.
 *   entries   a site with 7-mer q gives three, c = 0, 1, 2: entry c belongs to the 5-mer q[c, c + 5) (five plain bytes, no
 *             vocabulary), covers columns 3c, 3c + 1, 3c + 2 and carries n_reads[i]; ordered by site, then by c.
 *   sums      per entry and column s = colsum(v[0..n)) and s2 = colsum(v[i] * v[i]), every product rounded on its own, n the rows of
 *             the record.  colsum is np.sum of a Fortran-contiguous column: pieces of 8 192 elements, the first piece's sum, then
 *             each later piece's sum added in order; a piece is summed pairwise -- n < 8 sequentially from 0.0; 8 <= n <= 128 with
 *             eight accumulators r[j] = a[j], r[j] += a[i + j] for i = 8, 16, ... below n - n % 8, ((r0 + r1) + (r2 + r3)) +
 *             ((r4 + r5) + (r6 + r7)), then the last n % 8 elements one by one; n > 128 as the sum of the first n2 = n / 2 - (n / 2) % 8
 *             elements plus the sum of the rest (m6anet_amd/csrc/m6a_norm.h).
 *   fold      per 5-mer and column S and S2: the entries' sums added one by one in list order, from the first entry's; N the sum
 *             of n_reads (int64).  mean = S / N, std = sqrt(S2 / N - mean * mean), one IEEE operation each; a negative argument gives
 *             NaN.  Not pinned: the sign of a zero sum and the payload of a NaN.
 * Out, for the K 5-mers in bytewise order (K <= 3 n_sites, the capacity of every array): kmers [K][5], N [K], S, S2, mean, std
 * [K][3]; *n_kmers = K; status [n_sites] (may be NULL) 0 or the reason the kernels declined the site for; kmer7 [n_sites][7] (may be
 * NULL).  data.json goes up whole through the pinned chunk pair (M6A_PREP_CHUNK_KB) under the budget (M6A_PREP_BUDGET_MB, or free
 * memory less a margin), which also counts the rows' raw doubles (72 B per read); over it the call is M6A_ENOMEM and its text names
 * `--device cpu`.  Decline rule: that of m6a_json_sites_build less its two table checks.  Declined sites go, in ascending order,
 * through host->partials (m6a_io_norm_partials of libm6a_io.so) and their partial sums take their place before the fold; the
 * first one the loader does not parse ends the call with the loader's code (as M6A_EFORMAT / M6A_EIO) and text.  A row whose n_reads
 * is not the record's row count is M6A_EFORMAT "site <tx>:<pos>: data.info.labelled says <n> reads, data.json has <m>" (the
 * reference divides by the wrong count).  A status byte and the 7-mer per site and 64 bytes per 5-mer come back; nothing per read. */
typedef struct m6a_norm_host_half {
    int (*partials)(const char *json_path, int64_t n_sites, const char *tx_blob, const int64_t *tx_off, const int64_t *pos,
                    const int64_t *start, const int64_t *end, const int64_t *n_reads, const int64_t *sites, int64_t n, int n_threads,
                    double *s, double *s2, char *kmer7);
    const char *(*error)(void);
} m6a_norm_host_half;
typedef struct m6a_norm_stats {
    double ms_upload, ms_kernels, ms_host, ms_fold, ms_total;     /* ms_host: the declined sites */
    int64_t n_sites, n_reads, n_kmers, n_declined, d2h_bytes, peak_bytes;
} m6a_norm_stats;
int m6a_norm_factors_build(int device_id, const char *json_path, int64_t n_sites, const char *tx_blob, const int64_t *tx_off,
                           const int64_t *pos, const int64_t *start, const int64_t *end, const int64_t *n_reads,
                           const m6a_norm_host_half *host, int n_threads, char *kmers, int64_t *N, double *S, double *S2, double *mean,
                           double *std, int64_t *n_kmers, uint8_t *status, char *kmer7, m6a_norm_stats *stats);

/* data.site_proba.csv and data.indiv_proba.csv formatted on the device: the bytes m6a_io_write_csv_n writes (include/m6a_io.h),
 *   site row   <tx>,<pos>,<n_reads>,<%.16f of (double)site_prob>,<5-mer>,<%.16f of mod_ratio>\n
 *   read row   <tx>,<pos>,<id>,<%.16f of (double)read_prob>\n     <id> = <int>.0 when n_rep = 1, <int>_<replicate> when n_rep > 1
 * from arrays in device memory (the lengths of all rows, two exclusive 64-bit scans, then the text).  NaN and the infinities print as
 * glibc prints them (nan, -nan, inf, -inf).  The kernels DECLINE, and count, exactly: a finite probability or ratio that is negative
 * (-0.0 included) or >= 2; a read id that is not integral, is negative (-0.0 included) or is >= 10^15.  None of these comes out of
 * m6a_infer on an eventalign.txt whose read indices are below 10^15.  With anything declined a call returns M6A_EDECLINED, has written
 * no text and has opened no file; the caller writes through the host (m6a_io_write_csv_n).  Errors as the m6a_prep_* family: text in
 * m6a_prep_last_error(), M6A_EIO with the path for a file that cannot be opened or written, M6A_ENOMEM over the device budget.
 *
 * m6a_csv_format: HOST arrays in (the set m6a_io_sites_from_arrays_rep and m6a_io_write_csv_n take: kmer5 [S][5] without
 * terminators, read_rep [R] in [0, n_rep), read only when n_rep > 1), uploaded, the rows of sites [site_begin, site_end) formatted
 * on device device_id, the two texts out.  *site_bytes, *indiv_bytes and *n_declined are always set; with site_text = indiv_text =
 * NULL that is all (the sizing call), else both buffers must hold the texts.  Needs no weights and no m6a_ctx.
 *
 * m6a_prep_sites_write_csv: the same kernels on the handle's own device arrays after m6a_infer has filled read_prob / site_prob /
 * mod_ratio: the handle keeps the per-site transcript, position and 7-mer, the read ids and, for replicates, the per-site part
 * sizes on the device, and only the transcript names are uploaded.  Lengths and offsets are computed for the whole job first, so
 * both file sizes and the declined count are known before a file is opened or truncated.  Then the sites go in rounds of whole
 * sites bounded by M6A_CSV_ROUND_KB of text (default 32768; a site with more text than that is a round of its own), double-buffered
 * in pinned memory: round k + 1 is formatted and copied while round k is pwrite()n at its offsets by n_threads threads (0: the CPUs
 * this process may use).  write_header and n_sites_limit (< 0: all sites) as in m6a_io_write_csv_n.  stats (may be NULL) is filled
 * on every return; the handle's d2h_bytes grows by stats->d2h_bytes and its peak_bytes rises to the handle's arrays plus the writer's
 * buffers if that is higher. */
typedef struct m6a_csv_arrays {
    int64_t n_sites, n_tx;
    const int64_t *off;             /* [n_sites + 1], off[0] = 0 */
    const uint32_t *site_tx;        /* [n_sites] */
    const int64_t *site_pos;        /* [n_sites] */
    const char *kmer5;              /* [n_sites][5] */
    const char *tx_blob;
    const int64_t *tx_off;          /* [n_tx + 1] */
    const double *read_ids;         /* [R], R = off[n_sites] */
    const int32_t *read_rep;        /* [R], or NULL when n_rep = 1 */
    int n_rep;
    const float *read_prob, *site_prob;
    const double *mod_ratio;
} m6a_csv_arrays;
typedef struct m6a_csv_stats {
    double ms_format, ms_copy, ms_write;    /* lengths + scans + the write kernels; device -> pinned copies; pwrite */
    int64_t site_bytes, indiv_bytes;        /* text of either file, headers not counted */
    int64_t n_declined, d2h_bytes, n_rounds;
} m6a_csv_stats;
int m6a_csv_format(int device_id, const m6a_csv_arrays *a, int64_t site_begin, int64_t site_end, char *site_text, int64_t site_cap,
                   char *indiv_text, int64_t indiv_cap, int64_t *site_bytes, int64_t *indiv_bytes, int64_t *n_declined);
int m6a_prep_sites_write_csv(m6a_prep_sites *p, const char *out_dir, int write_header, int64_t n_sites_limit, int n_threads,
                             m6a_csv_stats *stats);

/* `dataprep --device gpu --writer device`: eventalign.index, data.json, data.info and data.log from arrays that never leave device
 * memory -- the bytes m6a_io_dataprep writes (include/m6a_io.h); tests/dataprep_json_statement.py states them in plain Python:
 *   data.json         per kept site {"<tx>":{"<pos>":{"<7-mer>":[[f,f,f,f,f,f,f,f,f,<read>.0],[...]]}}}\n  -- f = repr(float) of the nine
 *                     features in f64 (of np.round(f, 3) with `compress`), sites by transcript (order of first appearance), then
 *                     position, a site's reads in the order the host writer gives them
 *   eventalign.index  transcript_id,read_index,pos_start,pos_end\n, then <tx>,<read>,<start>,<end>\n per run, in file order
 *   data.info         transcript_id,transcript_position,start,end,n_reads\n, then <tx>,<pos>,<start>,<end>,<n_reads>\n per kept site:
 *                     [start, end) is the site's record in data.json
 *   data.log          <tx>: Data preparation ... Done.\n per transcript that passed the readcount cut with a candidate row
 * Numbers are printed by the core of m6anet_amd/csrc/m6a_repr.h, which DECLINES, and the kernels count: a feature that, after the
 * rounding of `compress`, is not a finite value with 1e-4 <= v < 1e16 (zero, negatives, what repr writes with an exponent, NaN, the
 * infinities), and a read index outside [0, 2^53).
 *
 * m6a_repr_format: HOST array in, every v[i] printed on device device_id (round3: np.round(v, 3) first), the texts out back to back:
 * value i is text[off[i], off[i + 1]); a declined value takes no bytes and is counted in *n_declined.  off [n + 1] and *n_declined are
 * always set; text = NULL is the sizing call, else cap must be >= off[n].  Needs no weights and no m6a_ctx.
 *
 * m6a_prep_dataprep_write: the back half of m6a_prep_sites_build under dataprep's rules (n_neighbors = 1; sites kept at
 * >= min_segment_count reads, no 20-read floor; no normalisation, no vocabulary; reads that disagree on a site's 7-mer are M6A_EFORMAT
 * with the host writer's text), then lengths (json_len_kernel, index_len_kernel), 64-bit scans -- both file sizes, every record's
 * [start, end) and the declined count are known before a file is opened -- and the text (json_write_kernel, index_write_kernel: a
 * wave stages text in LDS and stores aligned dwords) in rounds of whole sites / whole index rows bounded by M6A_JSON_ROUND_KB of text
 * (default 32768; a larger site is a round of its own), double-buffered in pinned memory and pwrite()n at their offsets by n_threads
 * threads (0: the CPUs this process may use).  Per kept site position, transcript, [start, end) and n_reads come back, per
 * transcript one byte; data.info and data.log are printed from them on the host.  Runs the front half declines go through `host`
 * as in m6a_prep_sites_build.  M6A_PREP_WINDOW_KB and M6A_PREP_CHUNK_KB as there; BGZF files and streams are refused (M6A_EINVAL).
 * With anything declined the call returns M6A_EDECLINED, has opened no file, and the caller writes through the host
 * (m6a_io_dataprep_write).  Other errors carry the host path's codes and texts (short line, no header, disagreeing sequence, missing
 * file); over the device budget is M6A_ENOMEM naming --device cpu.  On any error none of the four files is left behind.  stats (may
 * be NULL) is filled on every return. */
typedef struct m6a_dataprep_stats {
    double ms_front, ms_back, ms_format, ms_copy, ms_write;   /* front half; back half; lengths + scans + write kernels; device -> pinned; pwrite */
    int64_t json_bytes, index_bytes;                          /* sizes of data.json and eventalign.index (its header counted) */
    int64_t n_sites, n_runs, n_declined, n_rounds;            /* n_rounds: of data.json and of eventalign.index together */
    int64_t d2h_bytes, peak_bytes;
} m6a_dataprep_stats;
int m6a_repr_format(int device_id, const double *v, int64_t n, int round3, char *text, int64_t cap, int64_t *off /* [n + 1] */,
                    int64_t *n_declined);
int m6a_prep_dataprep_write(int device_id, const char *path, const char *out_dir, int readcount_min, int readcount_max,
                            int min_segment_count, int compress, const m6a_prep_host_half *host, int n_threads,
                            m6a_dataprep_stats *stats);

/* BGZF input (htslib's bgzip; SAM specification section 4.1).  m6a_prep_sites_build, _multi and _windows take a file of either kind,
 * and replicates may mix them; tests/bgzf_statement.py states the same in plain Python.
 *   detection    by content, never by name: a file whose first bytes are not 1f 8b is text and takes the path above untouched.  A file
 *                that starts 1f 8b but whose first member does not meet the header rules is refused, M6A_EFORMAT, with a text that says
 *                it is gzip but not BGZF and names `bgzip`.
 *   header       1f 8b 08 04, MTIME (4), XFL, OS, XLEN (2), then XLEN bytes of extra subfields SI1 SI2 SLEN (2) data, walked in order;
 *                the first with SI1 = 'B', SI2 = 'C', SLEN = 2 holds BSIZE = the block's total size - 1; others may stand before or
 *                after it.  The subfields must fill XLEN exactly and the block must have room for its footer.
 *   body         one raw DEFLATE stream (RFC 1951) of any number of stored, fixed and dynamic deflate blocks, then CRC32 (4) and
 *                ISIZE (4) <= 65536.  Blocks are independent: a distance never reaches before the first byte of its own block's
 *                output.  Empty blocks (ISIZE 0, such as the 28-byte end-of-file marker) may stand anywhere; a file without the
 *                marker is accepted, as htslib accepts it.
 *   text         the concatenation of the blocks' outputs; every byte offset in messages, runs and errors is an offset in it.
 *   errors       a bad header; a BSIZE that runs past the end of the file; ISIZE over 65536; deflate block type 3; a stored LEN/NLEN
 *                mismatch; a code-length set zlib refuses (over-subscribed; incomplete unless it is one code of one bit, never for the
 *                code-length code; no end-of-block code; more than 286 / 30 symbols; a repeat without a length before it or past the
 *                end); literal/length symbols 286-287, distance symbols 30-31 and codes no symbol has; a distance larger than the
 *                bytes produced so far in this block; output beyond ISIZE; input exhausted before the end-of-block code; a stream that
 *                does not end exactly at the footer; a length that is not ISIZE; a CRC-32 mismatch.  The first bad block in file
 *                order is reported, M6A_EFORMAT, `<path>: BGZF block at byte <file offset of the block>: <reason>`; nothing is
 *                parsed and no output file is touched.
 * The compressed bytes go up through the pinned chunks while the host walks the chain in them (BSIZE gives the next block), the text
 * buffer is allocated at the sum of ISIZE, one kernel inflates every block to its place and a second checks its CRC-32
 * (m6anet_amd/csrc/m6a_bgzf.h); one 8-byte status comes back, not a byte per block.  The compressed buffer counts against the budget
 * while it lives and is released before the line records are allocated.  What the host reads by path from a text file -- contig
 * names, the byte ranges of declined runs -- comes from the inflated text on the device in one gathered copy each (counted in
 * d2h_bytes); the host half gets the declined runs laid end to end in a temporary file, with offsets to match, which is removed.
 * Refused: windows over a BGZF file (window_bytes > 0 or M6A_PREP_WINDOW_KB > 0), M6A_EINVAL -- the file must fit resident; and
 * m6a_prep_eventalign on a BGZF file, M6A_EFORMAT naming eventalign_inference -- its eventalign.index would hold offsets into a
 * file that does not exist.
 *
 * m6a_bgzf_inflate: the text of a BGZF file, inflated on device device_id, into text[0, cap); *n_bytes is its length.  text == NULL
 * is the sizing call (the chain is walked on the host; nothing is uploaded).  Needs no weights and no m6a_ctx.  stats (may be NULL):
 * blocks, file bytes, the upload, the inflate kernel, the CRC kernel, the copy of the text to the host in ms, and d2h_bytes.  Errors
 * as the m6a_prep_* family, text in m6a_prep_last_error(). */
typedef struct m6a_bgzf_stats {
    int64_t n_blocks, compressed_bytes;
    double ms_upload, ms_inflate, ms_crc, ms_copy;
    int64_t d2h_bytes;
} m6a_bgzf_stats;
int m6a_bgzf_inflate(int device_id, const char *path, char *text, int64_t cap, int64_t *n_bytes, m6a_bgzf_stats *stats);

/* BGZF output: data.site_proba.csv.gz and data.indiv_proba.csv.gz deflated on the device (`eventalign_inference --compress`), files
 * that zcat, bgzip -d, pandas.read_csv and the reader above open.  tests/bgzf_statement.py reads what is written here.
 *   blocks       the text is cut into blocks of at most 65 280 bytes (0xff00, as htslib cuts them); a block is the 18-byte header
 *                1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 02 00 BSIZE, one raw DEFLATE stream, CRC32 and ISIZE.
 *   stream       one deflate block of fixed Huffman codes (BTYPE 01), or one stored block (BTYPE 00) when the coded stream would
 *                not be smaller than 5 + ISIZE bytes; so no BGZF block is larger than 65 536 bytes.
 *                This is level 1, what every entry point without a level writes.  Level 2 (`--compress_level 2`) is below.
 *   parts        the text of a block is cut into 64 parts of ceil(ISIZE / 64) bytes, each parsed greedily and on its own into
 *                literals and matches of 3..258 bytes.  A match starts and ends inside its part, and may reach back up to 256 bytes in
 *                front of the part (into earlier parts, never in front of the block).  The finder is a table of 128 x 2 positions
 *                per part, so the bytes depend on the text alone: the same text gives the same file on the host and on any device.
 *   file         the blocks, then the 28-byte end-of-file marker 1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 and
 *                eight zero bytes.  An empty text is the marker alone.
 * Level 2 keeps the blocks, the parts, the finder and so the tokens of level 1, and changes only how tokens become bits:
 *   counts       the block's counts of the literal/length symbols 0..285 and of the distance codes 0..29; end-of-block counts once.
 *   lengths      one prefix code per alphabet, of at most 15 bits: the used symbols sorted by (count, symbol), Moffat and Katajainen's
 *                in-place minimum-redundancy depths, depths over the limit cut to it and the Kraft sum repaired as zlib and miniz
 *                do (a code of the limit's length is dropped and one of the longest shorter codes becomes two codes a bit longer,
 *                until the sum is 1), the lengths dealt longest first to the rarest symbols.  The code is complete and costs what
 *                Huffman's costs where that fits the limit; a single used symbol gets length 1, and a block without a match sends
 *                one distance code of length 0 (RFC 1951, 3.2.7).  Codes are canonical.
 *   header       HLIT and HDIST drop the trailing unused symbols; the HLIT + HDIST lengths are one sequence, coded with 16 (3..6
 *                more of the same), 17 (3..10 zeros) and 18 (11..138 zeros, taken first) greedily; the code of those 19 symbols is
 *                built by the same rule with a limit of 7 bits.
 *   choice       the bits of the dynamic stream, header included, against those of the fixed stream: the smaller wins, fixed wins a
 *                tie, and a winner of 5 + ISIZE bytes or more is stored.  So a block is one deflate block of BTYPE 00, 01 or 10, never
 *                larger than level 1's block of the same text, and the bound and the 64 KiB slots hold.
 *   emission     as at level 1, with the dynamic header as one more bit string in front of part 0: offsets from the exclusive sum of
 *                the 65 lengths, one writer per byte, no byte read back.
 * A wave deflates a block, a lane a part, with the lanes' tables in LDS; the parts' bit strings are joined by an exclusive sum of
 * their lengths.  Blocks are written into slots of 64 KiB and packed by a scan and a second kernel (m6anet_amd/csrc/m6a_deflate.h);
 * one record of three words comes back per round -- the packed sizes and the stored blocks -- not a word per block.  At level 2 a
 * kernel of its own (bgzf_deflate_dyn_kernel) counts the parts' tokens into one histogram per wave with LDS atomics, lane 0 builds the
 * codes, and the record has a fourth word, the blocks of dynamic codes.
 *
 * m6a_bgzf_deflate: text[0, n) (host memory) deflated on device device_id into out[0, cap), *n_bytes its length, marker included; the
 * mirror of m6a_bgzf_inflate.  out == NULL is the sizing call: *n_bytes = ceil(n / 65280) * 65536 + 28, an upper bound, and no
 * device is touched.  Needs no weights and no m6a_ctx.  stats (may be NULL): blocks, stored blocks, the kernels and the copy of the
 * blocks to the host in ms, and d2h_bytes.  libm6a_io.so's m6a_io_bgzf_deflate gives the same bytes from the host.
 *
 * m6a_prep_sites_write_csv_bgzf: m6a_prep_sites_write_csv with the text deflated before it leaves the device.  Each round's two texts
 * are formatted as there, cut into blocks (a round ends its last block), deflated, packed, copied through the pinned pair and
 * pwrite()n at a running offset; round k + 1 is formatted and deflated while round k is copied and written.  With write_header the
 * header line is the first block of its file; without it the blocks go behind what the files hold.  Both files end with the marker.
 * The files are <out_dir>/data.site_proba.csv.gz and data.indiv_proba.csv.gz; the plain files are not created.  M6A_EDECLINED as for
 * the plain writer, before any file is opened; every device buffer -- text, slots and sizes of both rounds, which count in
 * peak_bytes and against the budget -- is allocated before that too, so M6A_ENOMEM leaves no file behind either. */
typedef struct m6a_deflate_stats {
    int64_t n_blocks, n_stored;
    double ms_deflate, ms_copy;
    int64_t d2h_bytes;
} m6a_deflate_stats;
int m6a_bgzf_deflate(int device_id, const char *text, int64_t n, char *out, int64_t cap, int64_t *n_bytes, m6a_deflate_stats *stats);
/* m6a_bgzf_deflate at level 1 (its bytes) or 2; another level is M6A_EINVAL.  n_by_type (may be NULL): blocks by BTYPE 0, 1, 2.
 * libm6a_io.so's m6a_io_bgzf_deflate_level gives the same bytes and counts from the host. */
int m6a_bgzf_deflate_level(int device_id, const char *text, int64_t n, int level, char *out, int64_t cap, int64_t *n_bytes,
                           m6a_deflate_stats *stats, int64_t n_by_type[3]);
typedef struct m6a_csv_bgzf_stats {
    double ms_format, ms_deflate, ms_copy, ms_write;    /* as m6a_csv_stats, and the three deflate kernels */
    int64_t site_bytes, indiv_bytes;                    /* text of either file, headers not counted */
    int64_t site_compressed, indiv_compressed;          /* bytes this call wrote to either file, header block and marker included */
    int64_t n_blocks, n_stored;                         /* BGZF blocks written (the marker not counted); those that came out stored */
    int64_t n_declined, d2h_bytes, n_rounds;
} m6a_csv_bgzf_stats;
int m6a_prep_sites_write_csv_bgzf(m6a_prep_sites *p, const char *out_dir, int write_header, int64_t n_sites_limit, int n_threads,
                                  m6a_csv_bgzf_stats *stats);
/* m6a_prep_sites_write_csv_bgzf at level 1 (its bytes) or 2; the header line's block is made by the host core at the same level.
 * n_by_type (may be NULL): the blocks written, header blocks included, by BTYPE 0, 1, 2. */
int m6a_prep_sites_write_csv_bgzf_level(m6a_prep_sites *p, const char *out_dir, int write_header, int64_t n_sites_limit, int n_threads,
                                        int level, m6a_csv_bgzf_stats *stats, int64_t n_by_type[3]);

/* `eventalign_inference --read_representation`: data.read_representation.npy written from the handle's device arrays -- X,
 * site_kmers and off never leave the device, and the process never holds more of the array than two rounds of it.
 *
 * The file is NumPy's .npy version 1.0 of a C-ordered [n_rows][32] array, n_rows = off[n], n = n_sites_limit (< 0: every site;
 * larger than the handle's count: every site), dtype '<f4' (M6A_REPR_F32) or '<f2' (M6A_REPR_F16).  Its header is byte for byte what
 * np.lib.format.open_memmap(path, mode="w+", dtype=np.float32 | np.float16, shape=(n_rows, 32)) writes (NumPy 1.24 and later):
 *     0x93 'N' 'U' 'M' 'P' 'Y' 0x01 0x00, then 0x76 0x00 (the little-endian length, 118, of what follows),
 *     {'descr': '<f4', 'fortran_order': False, 'shape': (<n_rows>, 32), }       ('<f2' for binary16)
 *     21 - (decimal digits of n_rows) spaces, which make dictionary and spaces 80 bytes at every n_rows,
 *     37 spaces and '\n'
 * -- 128 bytes, whatever n_rows is; tests/repr_file_statement.py states them in Python.  Row i follows at byte 128 + i * 32 *
 * itemsize and is what m6a_read_representation_dtype gives for read i: the row of data row i of data.indiv_proba.csv.
 *
 * Rounds of whole sites: a round takes as many sites as together have at most max(1, M6A_REPR_ROUND_KB * 1024 / (32 * itemsize))
 * rows (default 131072 KB), and at least one, so a site with more rows is a round of its own.  Two device buffers and two pinned
 * buffers of the largest round are allocated before the first round and none after it.  Round k's kernel runs on ctx's stream
 * straight from the handle's arrays; its device-to-host copy runs on a second stream behind an event; its pwrite() runs on the
 * host at the round's offset.  Round k + 1 is queued before round k's copy is waited for, so that copy runs under round k + 1's
 * kernel and round k - 1's pwrite().  The file is opened with O_TRUNC and sized once, before the first round.
 *
 * The four buffers count against the budget of the m6a_prep_* family (free device memory less a margin, or M6A_PREP_BUDGET_MB):
 * over it is M6A_ENOMEM with a text that names a smaller M6A_REPR_ROUND_KB.  The handle's d2h_bytes grows by the bytes copied
 * (n_rows * 32 * itemsize, stats->d2h_bytes) and its peak_bytes rises to the handle's arrays plus the buffers if that is higher.
 * M6A_EINVAL: p, ctx or path NULL; ctx on another device than p; a dtype that is neither constant; a handle with no site.
 * M6A_EIO with the path: the file cannot be opened, sized, written or closed.  A call that fails leaves no file at path.  Text in
 * m6a_prep_last_error().  ctx must be idle (no open job) and is left with nothing queued.  stats (may be NULL) is filled on every
 * return: the kernel and copy times are summed over the rounds from events, so with overlap they need not add up to the call. */
typedef struct m6a_repr_write_stats {
    double ms_kernel, ms_copy, ms_write;    /* the rounds' kernels; their device -> pinned copies; their pwrite()s */
    int64_t n_rounds, n_rows;
    int64_t bytes;                          /* the file: header and rows */
    int64_t round_bytes;                    /* each of the buffers: the largest round */
    int64_t d2h_bytes;
} m6a_repr_write_stats;
int m6a_prep_sites_write_read_representation(m6a_prep_sites *p, m6a_ctx *ctx, const char *path, int dtype, int64_t n_sites_limit,
                                             m6a_repr_write_stats *stats);

/* `train`: fitting the m6anet.toml model (m6anet/scripts/train.py -> train_one_epoch, m6anet/utils/training_utils.py; the model of
 * m6anet/model/configs/model_configs/m6anet.toml, which has no dropout, so a step is a deterministic function of its batch).  The
 * operation, stated once (tests/train_statement.py is the same in NumPy float64; the kernels of m6anet_amd/csrc/m6a_train.hip compute
 * it in float32).  One step on B bags of `bag` reads, N = B * bag reads:
 *   x    = [X (9) | E[k0] | E[k1] | E[k2]], 15 values;  z1 = W1 x + b1
 *   batch norm in training mode over the N reads: mu = mean(z1), var = the biased variance, xhat = (z1 - mu) / sqrt(var + 1e-5),
 *          y1 = gamma xhat + beta;  running_mean <- 0.9 running_mean + 0.1 mu;  running_var <- 0.9 running_var + 0.1 var N / (N - 1)
 *   a1   = relu(y1), a2 = relu(W2 a1 + b2), p = sigmoid(W3 a2 + b3)
 *   s_b  = 1 - prod_k (1 - p_bk), the product in float32, left to right, as m6a_bag_forward forms it
 *   loss = torch.nn.BCELoss(): the mean over the B sites of -(y max(log s, -100) + (1 - y) max(log(1 - s), -100)); its backward is
 *          dL/ds = (s - y) / max((1 - s) s, 1e-12) / B
 *   ds/dp_k = prod_{j != k} (1 - p_j), from the products before and behind read k -- nothing is divided by 1 - p_k, so a read with
 *          p = 1.0f gives its site the loss term 100 (y = 0) or 0 (y = 1) and a gradient of exactly zero
 *   clip (only after m6a_train_set_clip(max_norm > 0); the reference's clip_grad, torch.nn.utils.clip_grad_norm_ with the 2-norm,
 *          between backward() and the optimizer's step): total = sqrt(sum g^2) over the 7 697 trainable floats, the sum in float64
 *          in a fixed order, total in float32; coef = min(1, max_norm / (total + 1e-6)) in float32; g <- coef g, always multiplied
 *          (at coef = 1 no bit changes).  It comes after the gradient is complete and before Adam adds weight_decay theta.
 *   Adam as torch.optim.Adam applies it: g += weight_decay theta, m and v, theta -= lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *          over the 7 697 trainable floats E, W1, b1, gamma, beta, W2, b2, W3, b3; the two running statistics are not parameters.
 * Not built: the weighted loss, other topologies, more than one GPU.
 * Sums run in a fixed order and no float is added atomically: the same state and batch give the same bits.
 *
 *   m6a_train_create   weights: the 7 997-float blob of m6a_create (a HOST pointer, raw values); the trainer keeps its own copy, with
 *                      Adam's m and v at zero and t = 0, and never touches the context's inference layout.  cfg NULL = lr 4e-4, betas
 *                      0.9 / 0.999, eps 1e-8, weight_decay 0.  The trainer works on the context's device and stream (m6a_set_stream is
 *                      honoured) and must be destroyed before its context.
 *   m6a_train_step     X [n_bags * bag][9], site_kmers [n_bags][3], y [n_bags] (0 or 1), loss [1], y_pred [n_bags] = s (either may be
 *                      NULL).
 *   m6a_train_epoch    X / site_kmers / off / y describe n_sites sites as in m6a_infer.  Step k takes order[k * batch_size :
 *                      (k + 1) * batch_size]; the last batch may be short (DataLoader's drop_last=False).  Position i of `order`
 *                      draws its `bag` reads by the rule of m6anet_amd/csrc/m6a_train_draw.h and the kernels read X in place through
 *                      those indices: no batch is materialised.  loss [ceil(n_order / batch_size)], y_pred [n_order].  All steps
 *                      are queued back to back: the call waits for the stream once to learn that its arguments are valid (and once
 *                      more to deliver host outputs), however many steps there are.
 *   m6a_train_sample   the same indices on the host: read_idx [n_order * bag] global read numbers (off, order: host pointers).
 *   m6a_train_grads    the last step's gradient in blob order, zeros in the 300 running-statistic slots (before weight decay, as
 *                      torch's p.grad; with clipping on, the clipped gradient, as p.grad is after clip_grad_norm_).
 *   m6a_train_weights  the blob with the running statistics in place: it goes straight into m6a_create.  n_steps (may be NULL) = t.
 *   m6a_train_stats    steps taken, kernels launched, waits for the stream -- each may be NULL.  A step is 6 launches, 7 with
 *                      clipping on (the norm must be known in every block before Adam runs: one more kernel boundary); the waits
 *                      per call are the same either way.
 *   m6a_train_set_clip  max_norm of the clip above for every later step; 0 = off, the default, and then a step is what it is
 *                      on a trainer this was never called on, bit for bit.
 *   m6a_train_last_norm  the last step's `total`, from before the scaling.  M6A_EINVAL with clipping off (the default chain does
 *                      not compute the norm) and before the first step after m6a_train_set_clip.
 *   m6a_train_state_get  Adam's m and v (HOST pointers, M6A_N_WEIGHTS floats each in blob order, zeros in the 300
 *                      running-statistic slots) and t (n_steps, may be NULL).
 *   m6a_train_state_set  the inverse: on a trainer created from the blob m6a_train_weights gave, it makes the trainer that m, v and
 *                      t were taken from -- its next steps have that trainer's bits (the blob carries the running statistics).  The
 *                      running-statistic slots of m and v are stored as zeros.
 *
 * The step cut at s, for a caller that brings its own loss, sampler and optimizer (torch autograd: m6anet_amd/torch_model.py).
 * train_fwd2_kernel needs one number per site from the loss, dL/ds_b; everything behind that number -- the head, layer 2, batch norm
 * backward, the folds -- does not depend on which loss produced it.  So: forward returns s, backward takes dL/ds.
 *   m6a_train_set_weights  blob: 7 997 floats, a host or a device pointer, copied into the trainer's own blob (the running statistics
 *                      included); a device pointer is copied on the context's stream without a wait.  Adam's m, v and t are untouched.
 *                      The trainer's copy is what forward AND backward read: a caller that changes its own parameters between the
 *                      two still gets the gradient at the weights the forward ran on.  It ends the validity of an earlier ticket.
 *   m6a_train_forward  the first half of m6a_train_step and nothing else: train_fwd1_kernel, train_stats_kernel, then layer 2, the
 *                      head and the bag product (train_fwd2_kernel's forward instantiation).  s [n_bags] is m6a_train_step's y_pred
 *                      on the same weights and batch bit for bit, and so are the running statistics left in the trainer's blob: the
 *                      same arithmetic in the same order.  No loss, no gradient; Adam's state and n_steps do not move.  *ticket names
 *                      the activations kept in the trainer's scratch (the site_kmers are copied with them: the caller's buffers are
 *                      free again once the call's work has run); only the latest forward's are kept.  The argument checks and the
 *                      single wait of m6a_train_step, minus the labels.  training = 0 is M6A_EINVAL: eval mode is m6a_bag_forward's.
 *   m6a_train_running_stats  running_mean | running_var, 300 floats, out of the trainer's blob; a device pointer without a wait.
 *   m6a_train_backward  grad_s [n_bags] = dL/ds; grads: 7 997 floats in blob order, zeros in the 300 running-statistic slots, as
 *                      m6a_train_grads gives them (and m6a_train_grads gives these afterwards).  It queues the backward half: the head
 *                      and layer-2 backward from the kept activations with dL/ds read from memory (p is recomputed from the kept
 *                      layer-2 pre-activations, by the forward's operations: its bits), train_fold_kernel's two folds (its loss wave
 *                      runs over 0 sites), train_bwd1_kernel, train_grad_kernel's folds.  Layer 1 and the statistics do not run again:
 *                      the running statistics move once per forward, as in torch.  A ticket that is not the latest forward's is
 *                      M6A_EINVAL, and the text says what overwrote those activations (a later forward, a step or an epoch, new
 *                      weights, a larger batch).  The same ticket twice is allowed and gives the same bits (torch's retain_graph).
 *                      With device pointers it is stream-ordered with no wait.  What it computes is
 *                        dL/dlogit_bk = grad_s_b prod_{j != k} (1 - p_bj) (1 - p_bk) p_bk
 *                      and from there on the step's backward; there is no gradient with respect to X.
 * Pointers follow DATA POINTERS at the top; a host dataset is uploaded once per call, device-pointer calls are stream-ordered
 * after the one wait named above (m6a_sync before reading their outputs).
 * M6A_EINVAL: bag outside 1..M6A_MAX_SAMPLES; a batch of fewer than 2 reads (torch refuses a one-value batch norm) or of more than
 * 2^20; a site with fewer than `bag` reads; a k-mer id outside 0..65; an `order` entry outside [0, n_sites); a label that is not 0 or
 * 1; max_norm negative, NaN or infinite; a device pointer to m6a_train_state_get / _set; n_steps < 0; a v that is negative or not
 * finite, an m that is not finite.  Nothing is changed by a refused call. */
typedef struct m6a_trainer m6a_trainer;
typedef struct { float lr, beta1, beta2, eps, weight_decay; } m6a_train_config;
int m6a_train_create(m6a_ctx *ctx, const float *weights, size_t n_floats, const m6a_train_config *cfg, m6a_trainer **out);
void m6a_train_destroy(m6a_trainer *t);
int m6a_train_step(m6a_trainer *t, const float *X, const uint8_t *site_kmers, const float *y, int64_t n_bags, int bag,
                   float *loss, float *y_pred);
int m6a_train_epoch(m6a_trainer *t, const float *X, const uint8_t *site_kmers, const int64_t *off, const float *y, int64_t n_sites,
                    const int64_t *order, int64_t n_order, int64_t batch_size, int bag, uint64_t seed,
                    float *loss, float *y_pred);
int m6a_train_sample(const int64_t *off, const int64_t *order, int64_t n_order, int bag, uint64_t seed, int64_t *read_idx);
int m6a_train_grads(m6a_trainer *t, float *grads);
int m6a_train_weights(m6a_trainer *t, float *weights, int64_t *n_steps);
int m6a_train_stats(const m6a_trainer *t, int64_t *n_steps, int64_t *n_launches, int64_t *n_syncs);
int m6a_train_set_clip(m6a_trainer *t, float max_norm);   /* 0 = off (the default) */
int m6a_train_last_norm(m6a_trainer *t, float *total_norm);
int m6a_train_state_get(m6a_trainer *t, float *m, float *v, int64_t *n_steps);
int m6a_train_state_set(m6a_trainer *t, const float *m, const float *v, int64_t n_steps);
int m6a_train_set_weights(m6a_trainer *t, const float *blob);
int m6a_train_forward(m6a_trainer *t, const float *X, const uint8_t *site_kmers, int64_t n_bags, int bag, int training,
                      float *s, int64_t *ticket);
int m6a_train_running_stats(m6a_trainer *t, float *stats);
int m6a_train_backward(m6a_trainer *t, int64_t ticket, const float *grad_s, float *grads);

#ifdef __cplusplus
}
#endif
#endif
