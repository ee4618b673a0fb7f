/*
 * m6a_io.h -- C ABI of libm6a_io.so: the data formats either side of the hot path
 * (SURVEY.md section 8(f) ranks 1-2).  Host-only C++ (no HIP): usable without a GPU.
 *
 *   m6a_io_load_sites   replaces NanopolishDS / NanopolishReplicateDS.__getitem__ + inference_collate
 *                       for a whole job (m6anet/utils/data_utils.py:118-129,152-231,341-427,498-506):
 *                       data.info + data.json -> the flat arrays include/m6a.h takes.
 *   m6a_io_write_csv    replaces the row formatting of run_inference
 *                       (m6anet/utils/inference_utils.py:59-67): data.site_proba.csv /
 *                       data.indiv_proba.csv, byte-identical to the Python '%' formatting.
 *
 * Every function returns 0 or a negative code; m6a_io_last_error() has the text (thread-local).
 */
#ifndef M6A_IO_H
#define M6A_IO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct m6a_sites m6a_sites;

enum { M6A_IO_OK = 0, M6A_IO_EINVAL = -1, M6A_IO_ENOMEM = -2, M6A_IO_EIO = -3, M6A_IO_EFORMAT = -4 };

const char *m6a_io_last_error(void);

/* input_dirs: n_dirs directories, each holding data.info + data.json (one = single sample, several
 * = replicates: union of sites in order of first appearance, read counts summed, reads concatenated
 * in directory order, read ids printed "<id>_<replicate>").  Sites with fewer than min_reads reads are
 * dropped (data_utils.py:129).  Normalisation factors (data_utils.py:233-248): n_norm 5-mers
 * (norm_kmers = n_norm x 5 chars, no terminators) with mean/std [n_norm][3] in float64; features are
 * (x - mean) / std in float64, then float32.  n_norm = 0 disables normalisation.  n_threads <= 0:
 * all hardware threads. */
int m6a_io_load_sites(const char *const *input_dirs, int n_dirs, int min_reads,
                      const char *norm_kmers, const double *norm_mean, const double *norm_std, int n_norm,
                      int n_threads, m6a_sites **out);
void m6a_io_free(m6a_sites *s);

int64_t m6a_io_n_sites(const m6a_sites *s);
int64_t m6a_io_n_reads(const m6a_sites *s);
int m6a_io_n_replicates(const m6a_sites *s);
const float *m6a_io_X(const m6a_sites *s);                 /* [R][9] */
const uint8_t *m6a_io_site_kmers(const m6a_sites *s);      /* [S][3] vocabulary ids */
const int64_t *m6a_io_off(const m6a_sites *s);             /* [S+1] */
const int64_t *m6a_io_tx_pos(const m6a_sites *s);          /* [S] */
const double *m6a_io_read_ids(const m6a_sites *s);         /* [R] numeric read index */
const int32_t *m6a_io_read_rep(const m6a_sites *s);        /* [R] replicate of each read */
const char *m6a_io_tx_id(const m6a_sites *s, int64_t site);    /* NUL-terminated */
const char *m6a_io_kmer5(const m6a_sites *s, int64_t site);    /* centre 5-mer, NUL-terminated */
/* Sites for the writers only, from host arrays (`eventalign_inference`: m6a_prep_sites_build in include/m6a.h leaves X on the
 * device): off [S+1], tx_pos [S], site_tx [S] indexing the names tx_blob[tx_off[t], tx_off[t + 1]) (n_tx of them), kmer5 [S][5]
 * without terminators, read_ids [R]; one replicate.  m6a_io_X and m6a_io_site_kmers return NULL; m6a_io_write_csv / _n and the
 * shard writers print the rows m6a_io_load_sites' sites would print; m6a_io_save_store refuses them (M6A_IO_EINVAL: no features). */
int m6a_io_sites_from_arrays(int64_t n_sites, const int64_t *off, const int64_t *tx_pos, const char *tx_blob, const int64_t *tx_off,
                             int64_t n_tx, const uint32_t *site_tx, const char *kmer5, const double *read_ids, m6a_sites **out);
/* The same for n_rep pooled replicates (m6a_prep_sites_build_multi): read_rep [R] is each read's replicate, 0 <= read_rep[r] < n_rep.
 * With n_rep > 1 the writers print read ids as `<id>_<replicate>`, as for sites loaded from several input directories; m6a_io_read_rep
 * returns the copy; X and the k-mer ids are still absent and m6a_io_save_store still refuses. */
int m6a_io_sites_from_arrays_rep(int64_t n_sites, const int64_t *off, const int64_t *tx_pos, const char *tx_blob, const int64_t *tx_off,
                                 int64_t n_tx, const uint32_t *site_tx, const char *kmer5, const double *read_ids, const int32_t *read_rep,
                                 int n_rep, m6a_sites **out);
/* Read names on sites made by m6a_io_sites_from_arrays[_rep] (m6a_prep_sites_build_names, include/m6a.h): names16 holds 16 bytes per
 * name -- the 32 hex digits of the UUID, first digit first -- and replicate f's table is rows [name_off[f], name_off[f + 1]),
 * name_off [n_rep + 1] from 0, n_rep the sites' own.  Copied.  From then on every CSV writer, the _n and shard forms included,
 * prints the 36-byte UUID of row read_ids[r] of read r's replicate's table where it printed the number: `<uuid>` for one replicate,
 * `<uuid>_<replicate>` with n_rep > 1.  A read id that is not an integer inside its table is M6A_IO_EINVAL, here, and nothing is set.
 * m6a_io_uuid_parse / m6a_io_uuid_format: the core the HIP kernels compile (m6anet_amd/csrc/m6a_uuid.h) -- the field [p, p + n) as
 * 16 such bytes (returns 1) or refused (0: anything but 8-4-4-4-12 lowercase hex digits); 16 bytes as the 36, no terminator. */
int m6a_io_sites_set_read_names(m6a_sites *s, const uint8_t *names16, const int64_t *name_off, int n_rep);
int m6a_io_uuid_parse(const char *p, int64_t n, uint8_t *out16);
void m6a_io_uuid_format(const uint8_t *in16, char *out36);

/* Binary site store: everything m6a_io_load_sites produces -- normalised features,
 * k-mer ids, CSR offsets, ids -- in one file, so a dataset is parsed from data.json ONCE and every later run maps it
 * (replaces the per-item seek + json.loads + normalise of NanopolishDS.__getitem__, m6anet/utils/data_utils.py:
 * 152-231, written by m6anet/utils/dataprep_utils.py:473-485).  m6a_io_open_store maps the file read-only: the
 * arrays are views into the page cache, nothing is copied or parsed; the host-pointer path of m6a_infer streams X
 * from the mapping through its pinned ring.  `tag` (<= 63 chars) records what the features were normalised with;
 * m6a_io_store_tag returns it ("" for sites that came from m6a_io_load_sites). */
int m6a_io_save_store(const m6a_sites *s, const char *path, const char *tag);
int m6a_io_open_store(const char *path, m6a_sites **out);
const char *m6a_io_store_tag(const m6a_sites *s);

/* Appends the rows of all sites to <out_dir>/data.site_proba.csv and data.indiv_proba.csv
 * (headers are written when write_header != 0, truncating the files like
 * m6anet/scripts/inference.py:94-97).  read_prob [R], site_prob [S], mod_ratio [S]. */
int m6a_io_write_csv(const m6a_sites *s, const char *out_dir, const float *read_prob,
                     const float *site_prob, const double *mod_ratio, int write_header, int n_threads);
/* same, but only the first n_sites_limit sites (< 0: all): with m6a_reference_written_sites() (m6a.h) the files
 * hold exactly the rows the reference writes when its flush test leaves the last batches unwritten
 * (m6anet/utils/inference_utils.py:47) */
int m6a_io_write_csv_n(const m6a_sites *s, const char *out_dir, const float *read_prob,
                       const float *site_prob, const double *mod_ratio, int write_header, int n_threads,
                       int64_t n_sites_limit);

/* The same rows written by SEVERAL processes at once (`inference --gpus N`: every rank maps the same store and holds the
 * results of its own shard, so nobody has to collect the job's read probabilities -- 4 B per read -- just to print them):
 *   m6a_io_csv_shard_size    bytes the rows of sites [site_begin, site_end) take in each file (they are formatted and
 *                            counted; up to M6A_IO_CSV_KEEP_MB = 1024 MB of the text stays with the handle, and the
 *                            m6a_io_csv_shard_write that follows with the same range and arrays writes it instead of
 *                            formatting again); read_prob / site_prob / mod_ratio hold THAT range's values only;
 *   m6a_io_csv_shard_write   pwrite()s them at site_offset / indiv_offset (= header + the sizes of
 *                            all earlier shards, exchanged by the caller); the one rank with write_header != 0 also writes
 *                            both header lines and sets the files to their final sizes site_total / indiv_total
 *                            (< 0: leaves the size alone), which cuts whatever an earlier run left there;
 *   m6a_io_csv_header_bytes  length of the header line of data.site_proba.csv (which = 0) / data.indiv_proba.csv (1).
 * The bytes are those of m6a_io_write_csv over the whole job, whatever the cut (tests/test_host_io.py). */
int m6a_io_csv_shard_size(const m6a_sites *s, const float *read_prob, const float *site_prob, const double *mod_ratio,
                          int64_t site_begin, int64_t site_end, int n_threads, int64_t *site_bytes, int64_t *indiv_bytes);
int m6a_io_csv_shard_write(const m6a_sites *s, const char *out_dir, const float *read_prob, const float *site_prob,
                           const double *mod_ratio, int64_t site_begin, int64_t site_end, int n_threads,
                           int64_t site_offset, int64_t indiv_offset, int write_header, int64_t site_total, int64_t indiv_total);
int64_t m6a_io_csv_header_bytes(int which);

/* The writers' '%.16f' (inference_utils.py:62,66) without printf: same characters as snprintf("%.16f", v) for every
 * double (exact 128-bit arithmetic for 0 <= v < 2, snprintf itself otherwise); buf336 holds >= 336 bytes, NUL-terminated;
 * returns the length.  Exported so the tests can pin it against printf. */
int m6a_io_format_f16(double v, char *buf336);

/* How dataprep prints a float into data.json: Python's repr(float) -- what ujson / json.dump write in the reference
 * (dataprep_utils.py:473-480) -- shortest digits that round-trip, positional for 1e-4 <= |v| < 1e16, exponent form
 * otherwise.  buf40 holds >= 40 bytes, NUL-terminated; returns the length.  Exported so the tests can pin it against
 * Python's own repr. */
int m6a_io_py_repr(double v, char *buf40);
/* The writer's fast path for values np.round produced -- the mean (one decimal, dataprep_utils.py:293) and, with --compress,
 * every feature (three decimals): k / 10^digits written positionally with trailing zeros dropped, which IS repr() of such a
 * double for 0 < |v| < 1e9; returns the length, or -1 where the fast path declines (zero, huge, not the double nearest to
 * k / 10^digits, digits other than 1 or 3) and m6a_io_py_repr's general algorithm is used.  Exported for the tests. */
int m6a_io_repr_rounded(double v, int digits, char *buf40);
/* The number core the device writer of data.json compiles (m6anet_amd/csrc/m6a_repr.h), on the host: repr(v), or with round3
 * repr(np.round(v, 3)), for exactly the finite values with 1e-4 <= v < 1e16 after the rounding -- the bytes m6a_io_py_repr gives,
 * at most 24 of them, NUL-terminated.  Returns the length, or -1 where the core DECLINES (zero, negatives, below 1e-4, 1e16 and
 * above, NaN, the infinities; buf40 then holds an empty string).  Exported so the CPU tests reach the core without a GPU. */
int m6a_io_repr_core(double v, int round3, char *buf40);

/* `m6anet dataprep` (m6anet/scripts/dataprep.py:54-70 -> m6anet/utils/dataprep_utils.py):
 * eventalign.txt -> <out_dir>/eventalign.index (parallel_index, :187-266), data.json + data.info +
 * data.log (combine :269-325, filter_events :19-168, preprocess_tx :399-488).  Same arithmetic as
 * the reference on pandas >= 1.3 (Kahan-compensated group sums, np.round half-to-even, floats
 * printed as Python repr) and the reference's n_processes = 1 record order (transcripts in index
 * order, positions ascending); inside a position reads stay in index order (the reference's order
 * there comes from an unstable argsort and is machine-dependent).  n_neighbors = 1..16 flanking positions either side
 * (m6anet/scripts/dataprep.py:45-47; roll / partition_into_continuous_positions, dataprep_utils.py:51-67,117-147): rows
 * of 3 (2 n + 1) features and a (5 + 2 n)-mer; the shipped models take n_neighbors = 1.
 * skip_index != 0 reads an existing eventalign.index instead of rebuilding it.
 * Built for files of tens to hundreds of GB: the index is computed over byte ranges on all threads and stitched where a
 * read crosses a range boundary (one index row = one contiguous (contig, read_index) run; the reference sums the line
 * lengths of all rows of a key per chunk instead, which only differs for reads whose lines are not contiguous --
 * tests/golden/dataprep_noncontiguous pins that divergence); files over 2 GB (M6A_IO_POPULATE_MAX_MB) are mapped
 * lazily; a transcript's records are written as soon as every earlier transcript's are, so memory holds the index
 * (32 B per read) and at most M6A_IO_PENDING_MB (256) of finished-but-unwritten records, never the whole data.json.  M6A_IO_TRACE=1 prints
 * the phases. */
int m6a_io_dataprep(const char *eventalign_path, const char *out_dir, int n_threads,
                    int readcount_min, int readcount_max, int min_segment_count, int n_neighbors,
                    int compress, int skip_index);

/* The two halves of m6a_io_dataprep, for producers other than the host (`dataprep --device gpu`: m6a_prep_eventalign in
 * m6a.h returns the same table).  A table of plain arrays, owned by whoever made it:
 *   transcripts  name t = tx_blob[tx_off[t], tx_off[t + 1]), ids in order of first appearance;
 *   runs         the rows of eventalign.index in file order: run_tx, run_read, byte range [run_start, run_end);
 *                run_npos = number of combined (position, k-mer) groups; run_status M6A_PREP_RUN_OK, or M6A_PREP_RUN_HOST
 *                where the producer declined the run (a number outside the fast paths, events out of key order, a
 *                malformed line): m6a_io_dataprep_write combines it on the host, and its npos and rows are not read;
 *   rows         candidate windows, CSR by run (row_off[n_runs + 1]), in position order inside a run: row_pos = centre
 *                position (position + 2), row_kmer (5 + 2 n_neighbors) characters without terminator, row_feat
 *                3 (2 n_neighbors + 1) doubles, [dwell, sd, mean] per position from the first to the last of the window.
 * The candidate rows of a run are everything preprocess_tx derives from that run alone; the readcount cut, one run per
 * read (the last), n_pos > 1, the sort by position, min_segment_count and the text are m6a_io_dataprep_write's. */
enum { M6A_PREP_RUN_OK = 0, M6A_PREP_RUN_HOST = 1 };
typedef struct m6a_io_prep_table {
    int n_neighbors;
    int64_t n_tx;
    const char *tx_blob;
    const int64_t *tx_off;          /* [n_tx + 1] */
    int64_t n_runs;
    const uint32_t *run_tx;
    const int64_t *run_read, *run_start, *run_end, *run_npos;
    const int32_t *run_status;
    const int64_t *row_off;         /* [n_runs + 1] */
    int64_t n_rows;
    const int64_t *row_pos;
    const char *row_kmer;           /* [n_rows][5 + 2 n_neighbors] */
    const double *row_feat;         /* [n_rows][3 (2 n_neighbors + 1)] */
} m6a_io_prep_table;

typedef struct m6a_io_rows m6a_io_rows;
/* The table on the host: the index (or, with index_path non-NULL, the rows of that eventalign.index) and every run's
 * candidate rows (no run is declined).  Errors are those of m6a_io_dataprep's index phase. */
int m6a_io_dataprep_rows(const char *eventalign_path, const char *index_path, int n_threads, int n_neighbors, m6a_io_rows **out);
/* The rows of the given runs alone (byte ranges of eventalign_path, their read indices), as m6a_io_dataprep_rows makes them for its
 * own: a table of n_runs runs without transcripts, run_status M6A_PREP_RUN_HOST where a line is malformed.  The host half of
 * m6a_prep_sites_build (include/m6a.h: m6a_prep_host_half) for the runs its device front half declines. */
int m6a_io_runs_rows(const char *eventalign_path, int64_t n_runs, const int64_t *start, const int64_t *end, const int64_t *read,
                     int n_neighbors, int n_threads, m6a_io_rows **out);
const m6a_io_prep_table *m6a_io_rows_table(const m6a_io_rows *r);
void m6a_io_rows_free(m6a_io_rows *r);
/* The four files of m6a_io_dataprep from a table, whoever made it: eventalign.index from the runs (write_index != 0; with
 * skip_index the file is left as it is), data.json / data.info / data.log through the same per-transcript code.  Reads
 * eventalign_path only for the runs marked M6A_PREP_RUN_HOST. */
int m6a_io_dataprep_write(const char *eventalign_path, const char *out_dir, const m6a_io_prep_table *table, int n_threads,
                          int readcount_min, int readcount_max, int min_segment_count, int compress, int write_index);

/* A BGZF file (include/m6a.h states the format) inflated on the host by the decode core the HIP kernels compile
 * (m6anet_amd/csrc/m6a_bgzf.h): the text of all blocks into text[0, cap), its length in *n_bytes.  text == NULL is the sizing call:
 * *n_bytes is the sum of ISIZE over the chain as far as its headers can be walked, and nothing is inflated.  M6A_IO_EFORMAT with
 * `<path>: BGZF block at byte <offset>: <reason>` for the first bad block in file order (a bad header counts where it stands), with
 * its own text for a file that is not gzip, or is gzip but not BGZF. */
int m6a_io_bgzf_inflate(const char *path, char *text, int64_t cap, int64_t *n_bytes);

/* text[0, n) written as BGZF on the host by the deflate core the HIP kernels compile (m6anet_amd/csrc/m6a_deflate.h; include/m6a.h
 * states the writer): blocks of at most 65 280 text bytes, then the 28-byte end-of-file marker, into out[0, cap); the bytes are those
 * m6a_bgzf_deflate gives on a device.  out == NULL is the sizing call: *n_bytes = ceil(n / 65280) * 65536 + 28, an upper bound.
 * *n_stored (may be NULL): the blocks that came out stored. */
int m6a_io_bgzf_deflate(const char *text, int64_t n, char *out, int64_t cap, int64_t *n_bytes, int64_t *n_stored);

/* m6a_io_bgzf_deflate at a level of the writer (include/m6a.h states both): 1 gives m6a_io_bgzf_deflate's bytes, 2 codes every block
 * with the smaller of the fixed and its own Huffman codes; any other level is M6A_IO_EINVAL.  n_by_type (may be NULL): the blocks that
 * came out as deflate block type 0 (stored), 1 (fixed codes) and 2 (dynamic codes). */
int m6a_io_bgzf_deflate_level(const char *text, int64_t n, int level, char *out, int64_t cap, int64_t *n_bytes, int64_t n_by_type[3]);

/* The host half of m6a_json_sites_build (include/m6a.h: `inference --loader device`).
 * m6a_io_info_open: <dir>/data.info as m6a_io_load_sites reads it for one directory -- parse_info and the min_reads filter -- as a
 * table: the kept rows in file order with their transcript (names in order of first appearance), position, byte range and read
 * count.  A table without rows is not an error here.  The table is owned by the handle. */
typedef struct m6a_io_info m6a_io_info;
typedef struct m6a_io_info_table {
    int64_t n_sites, n_reads, n_tx;
    const uint32_t *site_tx;        /* [S] */
    const int64_t *pos, *start, *end, *site_reads;   /* [S] */
    const char *tx_blob;
    const int64_t *tx_off;          /* [n_tx + 1] */
} m6a_io_info_table;
int m6a_io_info_open(const char *dir, int min_reads, m6a_io_info **out);
const m6a_io_info_table *m6a_io_info_get(const m6a_io_info *info);
void m6a_io_info_free(m6a_io_info *info);
/* The rows of the table `sites` [n] names (ascending), through the per-site body of m6a_io_load_sites' workers: the range check,
 * the record, the 7-mer and 10 columns, "more reads than data.info says", the norm lookup, the count, the vocabulary.  X
 * [sum of their reads][9] and read_ids are the sites' rows laid end to end in list order, site_kmers [n][3], kmer7 [n][7].  On the
 * first failing site in list order the call returns the loader's code and text for it (what m6a_io_load_sites reports when that is the
 * lowest bad site of the directory) and the arrays are undefined.  data.json is mapped by the first call. */
int m6a_io_info_rows(m6a_io_info *info, const int64_t *sites, int64_t n, const char *norm_kmers, const double *norm_mean,
                     const double *norm_std, int n_norm, int n_threads, float *X, double *read_ids, uint8_t *site_kmers, char *kmer7);
/* One record through the decode core the kernels compile (m6anet_amd/csrc/m6a_json.h), on the host: 0 when the kernels take the
 * site (values [n_reads][10] and kmer7 [7] filled; either may be NULL), else the reason it is declined for, 1..14 in the order of
 * tests/json_statement.py's REASONS; M6A_IO_EINVAL for a null argument.  norm_kmers as m6a_io_load_sites takes them. */
int m6a_io_json_walk(const char *record, int64_t n, const char *tx, int64_t pos, int64_t n_reads, const char *norm_kmers, int n_norm,
                     double *values, char *kmer7);

/* `compute_norm_factors --device cpu`: the per-5-mer mean and std of the nine features over a list of sites, the operation
 * include/m6a.h states at m6a_norm_factors_build, on the host.
 * The site table is given as arrays of n_sites rows (the Train rows of data.info.labelled, in file order): row i is transcript
 * tx_blob[tx_off[i], tx_off[i + 1]) (tx_off holds n_sites + 1 ascending offsets), position pos[i], bytes [start[i], end[i]) of the
 * file json_path, n_reads[i] reads.  Every record goes through the loader's own per-site parser and its numbers stay doubles; the
 * loader's errors keep its code and text (range, JSON, 7-mer and 10 columns), and a row whose n_reads is not the record's row count is
 * M6A_IO_EFORMAT "site <tx>:<pos>: data.info.labelled says <n> reads, data.json has <m>".  The first failing row in table order is
 * reported.  No read-count filter, no vocabulary check.
 * m6a_io_norm_factors: threaded over the sites, folded in table order.  Out, for the K 5-mers in bytewise order (K <= 3 n_sites, the
 * capacity every array must have): kmers [K][5], N [K], S [K][3], S2 [K][3], mean [K][3], std [K][3]; *n_kmers = K; kmer7 [n_sites][7]
 * (may be NULL) the sites' 7-mers.
 * m6a_io_norm_partials: the host half of m6a_norm_factors_build -- s [n][9], s2 [n][9] (column sums of the values and of their squares,
 * in np.sum's order) and kmer7 [n][7] of the rows `sites` [n] names (ascending; NULL with n = n_sites: all of them). */
int m6a_io_norm_factors(const char *json_path, int64_t n_sites, const char *tx_blob, const int64_t *tx_off, const int64_t *pos,
                        const int64_t *start, const int64_t *end, const int64_t *n_reads, int n_threads, char *kmers, int64_t *N, double *S,
                        double *S2, double *mean, double *std, int64_t *n_kmers, char *kmer7);
int m6a_io_norm_partials(const char *json_path, int64_t n_sites, const char *tx_blob, const int64_t *tx_off, const int64_t *pos,
                         const int64_t *start, const int64_t *end, const int64_t *n_reads, const int64_t *sites, int64_t n, int n_threads,
                         double *s, double *s2, char *kmer7);

/* m6a_site_ranksum (include/m6a.h states the operation) on the host: the same arguments without the context, every array a host
 * array, the pairs spread over n_threads threads (0: the usable CPUs).  The counts and z are the kernel's, bit for bit: both compile
 * m6anet_amd/csrc/m6a_ranksum.h.  A pair is counted from sorted copies of its two bags, so the cost is O((n + m) log(n + m)).
 * pair_a and pair_b may be NULL (the identity: n_pairs == n_sites_a == n_sites_b); gt, eq and tie may each be NULL; z is required.
 * M6A_IO_EINVAL, with the outputs untouched, for a null required pointer, a negative count, offsets that do not start at 0 or that
 * decrease, and a pair index outside its set.  n_pairs == 0 is M6A_IO_OK. */
int m6a_io_site_ranksum(const float *prob_a, const int64_t *off_a, int64_t n_sites_a, const float *prob_b, const int64_t *off_b,
                        int64_t n_sites_b, const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs, int64_t *gt, int64_t *eq,
                        int64_t *tie, double *z, int n_threads);
/* m6a_site_signal_ranksum (include/m6a.h) on the host: X_* [off_*[n_sites_*]][9], outputs [n_pairs][9].  Per pair and column, the column
 * of either bag is gathered into scratch and counted by m6a_ranksum.h's count(), so a NaN leaves its own column undefined and no other;
 * arguments, errors and threading are m6a_io_site_ranksum's. */
int m6a_io_site_signal_ranksum(const float *X_a, const int64_t *off_a, int64_t n_sites_a, const float *X_b, const int64_t *off_b,
                               int64_t n_sites_b, const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs, int64_t *gt, int64_t *eq,
                               int64_t *tie, double *z, int n_threads);
/* m6a_site_ks and m6a_site_signal_ks (include/m6a.h state the operation) on the host: the two Kolmogorov-Smirnov integers and the two
 * medians per pair (per pair and column: X_* [off_*[n_sites_*]][9], outputs [n_pairs][9]), the kernels' bits -- both sides compile
 * m6anet_amd/csrc/m6a_ks.h, which counts a pair from sorted copies of its two bags.  d_pos and d_neg are required, med_a and med_b may
 * each be NULL; everything else -- arguments, errors with the outputs untouched, threading -- is m6a_io_site_ranksum's. */
int m6a_io_site_ks(const float *prob_a, const int64_t *off_a, int64_t n_sites_a, const float *prob_b, const int64_t *off_b,
                   int64_t n_sites_b, const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs, int64_t *d_pos, int64_t *d_neg,
                   double *med_a, double *med_b, int n_threads);
int m6a_io_site_signal_ks(const float *X_a, const int64_t *off_a, int64_t n_sites_a, const float *X_b, const int64_t *off_b,
                          int64_t n_sites_b, const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs, int64_t *d_pos, int64_t *d_neg,
                          double *med_a, double *med_b, int n_threads);
/* m6a_ks_exact (include/m6a.h states the recurrence, the caps and what is undefined) on the host: p[k] is the exact two-sided
 * Kolmogorov-Smirnov p-value of item (n[k], m[k], h[k]), NaN where it is undefined, the kernel's bits -- both sides compile
 * m6anet_amd/csrc/m6a_ks_exact.h.  One row of min(n, m) + 2 doubles, only the cells inside the band computed.  count == 0 is
 * M6A_IO_OK; a null pointer or a negative count is M6A_IO_EINVAL with p untouched. */
int m6a_io_ks_exact(const int64_t *n, const int64_t *m, const int64_t *h, int64_t count, double *p);

#ifdef __cplusplus
}
#endif
#endif
