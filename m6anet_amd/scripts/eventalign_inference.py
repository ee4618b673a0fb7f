"""`eventalign_inference` sub-command: eventalign.txt -> data.site_proba.csv / data.indiv_proba.csv in one process, byte-identical
to `dataprep --device cpu` followed by `inference` with the same flags.  The file is parsed, combined and windowed in HBM
(m6a_prep_sites_build, include/m6a.h), the sites' features go from there to X without leaving the device, and only ids and
probabilities come back to the host; no data.json is written or parsed.  With --grouped (m6a_prep_group) the sites come in batches as
transcripts complete, each scored and appended to the two files while the input still arrives (main_grouped)."""
import os
import pathlib
import time
from argparse import Action, ArgumentDefaultsHelpFormatter, ArgumentParser

from . import dataprep, inference

# the flags of `dataprep` that shape the sites, and every flag of `inference` but its input and --gpus (same defaults and meaning)
DATAPREP_FLAGS = ("--readcount_min", "--readcount_max", "--min_segment_count", "--n_processes")
INFERENCE_FLAGS = ("--pretrained_model", "--model_config", "--model_state_dict", "--norm_path", "--batch_size", "--save_per_batch",
                   "--num_iterations", "--device", "--seed", "--read_proba_threshold", "--encoder", "--drop_unflushed_tail")


def _copy(src, dst, flags):
    for a in src._actions:
        if any(o in flags for o in a.option_strings):
            dst._add_action(a)


class OneOrSeveral(Action):
    """--eventalign a.txt -> "a.txt" (one file, as ever); --eventalign a.txt b.txt -> ["a.txt", "b.txt"] (replicates)."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values[0] if len(values) == 1 else list(values))


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    parser.add_argument("--eventalign", required=True, nargs="+", action=OneOrSeveral,
                        help="eventalign filepath, the output from nanopolish; plain text or BGZF (bgzip) -- told apart by content, "
                             "inflated on the device, and replicates may mix the two.  Several files are replicates: their sites are pooled "
                             "as `inference` pools several --input_dir (a site is kept when its reads summed over the files reach 20), "
                             "and read ids are written <id>_<position of the file>.  `-` is the standard input, and a path that is no "
                             "regular file (a FIFO, a process substitution) is read as a stream too: `f5c eventalign ... | m6anet_amd "
                             "eventalign_inference --eventalign - ...` needs no eventalign file on disk.  A stream is plain text (inflate "
                             "a compressed one on the way: `bgzip -dc FILE |`), is read once and in order, always in windows (--window_mb), "
                             "and gives the bytes the same text in a file gives; replicates may mix files and streams, `-` once.")
    parser.add_argument("--out_dir", required=True, help="directory to output inference results.")
    _copy(dataprep.argparser(), parser, DATAPREP_FLAGS)
    _copy(inference.argparser(), parser, INFERENCE_FLAGS)
    return parser


def cli_parser():
    """argparser() -- the flags this command shares with `dataprep` and `inference` -- and the flag that is its own"""
    parser = argparser()
    parser.add_argument("--csv", choices=("host", "device"), default="host",
                        help="who formats the rows of the two CSV files: the host's threads from the probabilities copied back, or HIP "
                             "kernels from the arrays in device memory, the text coming back in pinned rounds (about 50 B per read "
                             "cross the link instead of 13).  The bytes are the same; values the kernels decline go through the host.")
    parser.add_argument("--window_mb", type=int, default=0,
                        help="parse each eventalign file in windows of this many MB instead of keeping all of it in device memory "
                             "(0: the whole file, about 3 bytes of device memory per byte of text -- unless M6A_PREP_WINDOW_KB is set, which 0 leaves in force).  With windows the device "
                             "holds two windows and the candidate rows, so a file larger than device memory goes through; the bytes "
                             "written are the same.  A stream (--eventalign -, a FIFO) is always parsed in windows: of this size, or of "
                             "256 MB with neither this flag nor the variable set.")
    parser.add_argument("--compress", action="store_true",
                        help="write data.site_proba.csv.gz and data.indiv_proba.csv.gz (BGZF: zcat, bgzip -d and pandas.read_csv open "
                             "them) instead of the two plain files; the text inside is the same.  With --csv device the text is deflated "
                             "by HIP kernels before it crosses the link (about a third of the bytes); with --csv host, and for values "
                             "the kernels decline, the host compresses the text it formatted.")
    parser.add_argument("--compress_level", type=int, choices=(1, 2), default=1,
                        help="with --compress and --csv device: 1 codes every BGZF block with the fixed Huffman codes of RFC 1951, "
                             "2 gives every block its own (dynamic) codes where they are smaller -- the same parse, about 0.6 of "
                             "level 1's bytes on the CSV text.  The host route (--csv host, declined values) is zlib, which writes "
                             "dynamic codes at any level, so there the flag changes nothing.  Without --compress it is an error.")
    parser.add_argument("--read_names", action="store_true",
                        help="column 4 of every eventalign file is the read's name, a lowercase UUID, as nanopolish and f5c write it with "
                             "--print-read-names (xPore and nanocompore need that form), not the integer read_index.  Runs are keyed by "
                             "the 128-bit name, the names are interned on the device, and data.indiv_proba.csv carries the UUID (or "
                             "<uuid>_<position of the file> with replicates) in its read_index column; every other byte is what the same "
                             "file with indices gives.  Anything else in that column is an error.  Only this command has the flag: "
                             "data.json stores the read id as a number and cannot hold a name, so `dataprep` and `inference` cannot carry one.")
    return parser


def command_parser():
    """cli_parser() and `inference`'s --site_proba: the parser of the `eventalign_inference` command"""
    return inference.add_site_proba(cli_parser())


def full_parser():
    """command_parser() and the two flags of the read representation: the parser of the `eventalign_inference` command"""
    parser = command_parser()
    parser.add_argument("--read_representation", action="store_true",
                        help="also write OUT_DIR/%s: [n_reads][32], the read encoder's output -- layer 2 after its ReLU, what the "
                             "reference's MILModel.get_read_representation returns, bit for bit -- one row per data row of "
                             "data.indiv_proba.csv, in its order: the bytes `dataprep` and `inference --read_representation` write for the "
                             "same text.  It is computed from the features in device memory after the CSV files are written, in rounds "
                             "(M6A_REPR_ROUND_KB, default 131072) whose copies and writes overlap the next round's kernel, so neither "
                             "data.json nor the whole array is ever held.  Works with every other flag; --compress leaves it a plain "
                             ".npy, and with --drop_unflushed_tail it has the rows the CSV has." % inference.REPR_FILE)
    return inference.add_representation_dtype(parser)


def grouped_parser():
    """full_parser() and --grouped: the parser of the `eventalign_inference` command"""
    parser = full_parser()
    parser.add_argument("--grouped", action="store_true",
                        help="the file's transcripts each form one stretch, as nanopolish and f5c write them from a coordinate-sorted BAM: "
                             "the sites of a transcript are built, scored and written once another contig follows it, and its runs and rows "
                             "are released, so device memory follows the window (--window_mb; 256 MB with neither the flag nor "
                             "M6A_PREP_WINDOW_KB set, for regular files too) and the group size (M6A_PREP_GROUP_KB, default 262144), not the "
                             "file, and the CSV files grow while the input -- a file, `-`, a FIFO -- still arrives.  Both CSV files are byte "
                             "for byte those of the command without the flag.  Input that is not grouped is an error that names the "
                             "transcript and the byte where it appears again, and leaves no CSV file.  One plain-text file; not with "
                             "--read_names, --compress or --read_representation.")
    return parser


# what --grouped does not take, each refused as an argument error (exit status 2) before anything is opened
GROUPED_REFUSALS = (
    (lambda a: not isinstance(a.eventalign, (str, bytes, os.PathLike)),
     "--grouped takes one --eventalign file: replicates are pooled over whole files, which a batch of transcripts is not"),
    (lambda a: getattr(a, "read_names", False),
     "--grouped with --read_names is not built: read names are interned over the whole file after its last window"),
    (lambda a: getattr(a, "compress", False),
     "--grouped with --compress is not built: a BGZF file cannot be appended to behind its end-of-file block"),
    (lambda a: getattr(a, "read_representation", False),
     "--grouped with --read_representation is not built: the .npy header states the number of rows, which is known at the end"),
)


GZ = ("data.site_proba.csv", "data.indiv_proba.csv")


def write_on_host_compressed(writer, out_dir, read_prob, site_prob, mod_ratio, n_threads, n_sites):
    """--compress without the kernels: the host writer's two files, formatted into a directory of their own under out_dir, then
    written as BGZF next to it (m6anet_amd/bgzf.py, zlib in threads) and removed.  Returns the bytes of the two .gz files."""
    import shutil
    import tempfile

    from .. import _io, bgzf
    tmp = tempfile.mkdtemp(prefix=".csv_plain_", dir=out_dir)
    try:
        writer.write_csv(tmp, read_prob, site_prob, mod_ratio, write_header=True, n_threads=n_threads, n_sites=n_sites)
        workers = n_threads if n_threads > 0 else _io.usable_cpus()
        return sum(bgzf.compress_file(os.path.join(tmp, fn), os.path.join(out_dir, fn + ".gz"), n_processes=workers, span_blocks=64,
                                      threads=True)[1] for fn in GZ)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def write_on_device(sites, out_dir, n_threads, n_sites, compress=False, level=1):
    """--csv device: prep_sites.write_csv's statistics, or None after one line on stderr when the kernels declined a value --
    nothing has been opened or written then, and the caller writes the same bytes through the host."""
    import sys

    from .. import _io
    try:
        return sites.write_csv(out_dir, write_header=True, n_threads=n_threads, n_sites=n_sites, **({"compress": True} if compress else {}),
                               **({"level": level} if compress and level != 1 else {}))
    except _io.CsvDeclined as e:
        print("eventalign_inference: --csv device declined %d values (%s); writing the CSV files on the host"
              % (e.n_declined, str(e).split(": ", 1)[1]), file=sys.stderr, flush=True)
        return None


def main_grouped(args, weights, device, csv_on, window_mb):
    """--grouped: the loop over the batches of _io.prep_sites_grouped.  Every batch starts on a flush-group boundary of the job, so the
    engine scores it under set_job_offset(first_site) as it scores those sites in the whole job, and the chosen writer appends its
    rows; the header goes with the first batch.  An error that comes once rows were written removes both CSV files: a CSV that
    exists is complete."""
    import sys
    import threading

    import numpy as np

    from .. import _io
    from ..constants import DEFAULT_MIN_READS, N_SAMPLES
    from ..data_utils import load_norm_factors
    from ..engine import reference_written_sites

    t_start = time.perf_counter()
    made = {}

    def make_engine():                       # the GPU context comes up while the first windows are parsed
        try:
            made["engine"] = inference.make_engine_for(args, weights, device)
        except BaseException as exc:        # re-raised on the main thread below
            made["error"] = exc

    starter = threading.Thread(target=make_engine)
    starter.start()
    try:
        group = _io.prep_sites_grouped(args.eventalign, args.readcount_min, args.readcount_max, args.min_segment_count,
                                       load_norm_factors(args.norm_path), args.n_processes, device,
                                       window_kb=window_mb * 1024 if window_mb else None, batch_size=args.batch_size,
                                       save_per_batch=args.save_per_batch)
    finally:
        starter.join()
    if "error" in made:
        group.close()
        raise made["error"]
    engine = made["engine"]
    wrote = False
    ms = {"infer": 0.0, "csv_write": 0.0, "first_csv_byte": None}
    n_sites = n_reads = 0
    try:
        pathlib.Path(args.out_dir).mkdir(parents=True, exist_ok=True)
        for sites in group:
            i = sites.info
            t0 = time.perf_counter()
            engine.set_job_offset(group.first_site)
            engine.set_host_offsets(sites.off)
            engine.infer_ptrs(i.X, i.site_kmers, i.off, sites.n_sites, args.num_iterations, N_SAMPLES, args.read_proba_threshold, args.seed,
                              args.batch_size, args.save_per_batch, i.read_prob, i.site_prob, i.mod_ratio)
            engine.sync()
            t1 = time.perf_counter()
            n_write = None
            if args.drop_unflushed_tail:     # the reference's row set of the job so far, less what the batches before have written
                n_write = reference_written_sites(group.first_site + sites.n_sites, args.batch_size, args.save_per_batch) - group.first_site
            done = False
            if csv_on == "device":
                try:
                    sites.write_csv(args.out_dir, write_header=not wrote, n_threads=args.n_processes, n_sites=n_write)
                    done = True
                except _io.CsvDeclined as e:
                    print("eventalign_inference: --csv device declined %d values (%s); writing the batch's rows on the host"
                          % (e.n_declined, str(e).split(": ", 1)[1]), file=sys.stderr, flush=True)
            if not done:
                read_prob, site_prob, mod_ratio = sites.fetch()
                writer = sites.writer()
                try:
                    writer.write_csv(args.out_dir, read_prob, site_prob, mod_ratio, write_header=not wrote, n_threads=args.n_processes,
                                     n_sites=n_write)
                finally:
                    writer.close()
            wrote = True
            t2 = time.perf_counter()
            if ms["first_csv_byte"] is None:
                ms["first_csv_byte"] = (t2 - t_start) * 1e3
            ms["infer"] += (t1 - t0) * 1e3
            ms["csv_write"] += (t2 - t1) * 1e3
            n_sites += sites.n_sites
            n_reads += sites.n_reads
        if not wrote:                        # what the default leaves behind: the two header lines, then the loader's error
            empty = _io.NativeSites.from_arrays(np.zeros(1, np.int64), np.zeros(0, np.int64), b"", np.zeros(1, np.int64), np.zeros(0, np.uint32),
                                                np.zeros((0, 5), np.uint8), np.zeros(0))
            try:
                empty.write_csv(args.out_dir, [], [], [], write_header=True, n_threads=args.n_processes)
            finally:
                empty.close()
            raise _io.M6AIOError("m6a_io error -4: no site with at least %d reads" % DEFAULT_MIN_READS, -4)
        if os.environ.get("M6A_EVENTALIGN_TIMES"):      # for tools/measure_eventalign_inference.py
            import json
            c = group.counts()
            ms["total"] = (time.perf_counter() - t_start) * 1e3
            print("M6A_TIMES " + json.dumps({"ms": ms, "d2h_bytes": c["d2h_bytes"], "n_sites": n_sites, "n_reads": n_reads, "csv_writer": csv_on,
                                                "n_windows": c["n_windows"], "window_bytes": c["window_bytes"], "peak_bytes": c["peak_bytes"],
                                                "stream_bytes": c["stream_bytes"], "n_streams": 1 if c["stream_bytes"] else 0,
                                                "n_batches": c["n_batches"], "max_kept_rows": c["max_kept_rows"],
                                                "max_kept_runs": c["max_kept_runs"], "group_bytes": c["group_bytes"],
                                                "total_rows": c["total_rows"], "total_runs": c["total_runs"]}), flush=True)
    except BaseException:
        if wrote:
            for fn in GZ:
                try:
                    os.remove(os.path.join(args.out_dir, fn))
                except OSError:
                    pass
        raise
    finally:
        group.close()
        engine.close()


def main(args):
    import threading

    from .. import _io
    from ..constants import DEFAULT_MIN_READS, N_SAMPLES
    from ..data_utils import load_norm_factors
    from ..engine import reference_written_sites

    if getattr(args, "compress_level", 1) != 1 and not getattr(args, "compress", False):       # an argument error, before anything is touched
        import sys
        print("m6anet_amd eventalign_inference: error: --compress_level %d needs --compress" % args.compress_level, file=sys.stderr)
        raise SystemExit(2)
    if getattr(args, "grouped", False):
        import sys
        for refused, text in GROUPED_REFUSALS:
            if refused(args):
                print("m6anet_amd eventalign_inference: error: " + text, file=sys.stderr)
                raise SystemExit(2)
    inference.check_representation_dtype(args, "eventalign_inference")
    weights = inference.resolve_model(args)
    device = inference._device_index(args.device)
    csv_on = getattr(args, "csv", "host")    # argparser() alone (no --csv): the host writer
    window_mb = getattr(args, "window_mb", 0)
    compress = getattr(args, "compress", False)
    level = getattr(args, "compress_level", 1)
    read_names = getattr(args, "read_names", False)
    want_repr = getattr(args, "read_representation", False)
    if window_mb < 0:
        raise ValueError("--window_mb must be 0 or more, not %d" % window_mb)
    if getattr(args, "grouped", False):
        return main_grouped(args, weights, device, csv_on, window_mb)
    made = {}

    def make_engine():                       # the GPU context comes up while the file is parsed
        try:
            made["engine"] = inference.make_engine_for(args, weights, device)
        except BaseException as exc:        # re-raised on the main thread below
            made["error"] = exc

    starter = threading.Thread(target=make_engine)
    starter.start()
    try:
        sites = _io.prep_sites(args.eventalign, args.readcount_min, args.readcount_max, args.min_segment_count,
                               load_norm_factors(args.norm_path), args.n_processes, device,
                               window_kb=window_mb * 1024 if window_mb else None, **({"read_names": True} if read_names else {}))
    finally:
        starter.join()
    if "error" in made:
        sites.close()
        raise made["error"]
    engine = made["engine"]
    try:
        pathlib.Path(args.out_dir).mkdir(parents=True, exist_ok=True)
        writer = sites.writer() if csv_on == "host" or sites.n_sites == 0 else None       # --csv device needs it only to fall back
        if sites.n_sites == 0:               # what `inference` leaves behind: the two header lines, then the loader's error
            if compress:
                write_on_host_compressed(writer, args.out_dir, [], [], [], args.n_processes, None)
            else:
                writer.write_csv(args.out_dir, [], [], [], write_header=True, n_threads=args.n_processes)
            raise _io.M6AIOError("m6a_io error -4: no site with at least %d reads" % DEFAULT_MIN_READS, -4)
        i = sites.info
        t0 = time.perf_counter()
        engine.set_host_offsets(sites.off)   # the kernels are chosen from this copy: nothing is read back
        engine.infer_ptrs(i.X, i.site_kmers, i.off, sites.n_sites, args.num_iterations, N_SAMPLES, args.read_proba_threshold, args.seed,
                          args.batch_size, args.save_per_batch, i.read_prob, i.site_prob, i.mod_ratio)
        engine.sync()
        t1 = time.perf_counter()
        n_write = None
        if args.drop_unflushed_tail:         # the reference's row set (inference_utils.py:47)
            n_write = reference_written_sites(sites.n_sites, args.batch_size, args.save_per_batch)
        csv = write_on_device(sites, args.out_dir, args.n_processes, n_write, compress, level) if csv_on == "device" else None
        t2 = time.perf_counter()
        host_gz = None
        if csv is None:
            read_prob, site_prob, mod_ratio = sites.fetch()
            t2 = time.perf_counter()
            writer = writer or sites.writer()
            if compress:
                host_gz = write_on_host_compressed(writer, args.out_dir, read_prob, site_prob, mod_ratio, args.n_processes, n_write)
            else:
                writer.write_csv(args.out_dir, read_prob, site_prob, mod_ratio, write_header=True, n_threads=args.n_processes, n_sites=n_write)
        t3 = time.perf_counter()
        rep = {"n_rounds": 0, "bytes": 0, "ms_kernel": 0.0, "ms_copy": 0.0, "ms_write": 0.0}
        if want_repr:                        # after the CSV files: X, site_kmers and off are still where infer_ptrs read them
            rep = sites.write_read_representation(engine, os.path.join(args.out_dir, inference.REPR_FILE),
                                                  getattr(args, "representation_dtype", "float32"), n_write)
        if os.environ.get("M6A_EVENTALIGN_TIMES"):      # phases for tools/measure_eventalign_inference.py
            import json
            ms, d2h = sites.times()
            ms.update(intern=sites.ms_intern)
            ms.update(repr_kernel=rep["ms_kernel"], repr_copy=rep["ms_copy"], repr_write=rep["ms_write"],
                      repr_total=(time.perf_counter() - t3) * 1e3 if want_repr else 0.0)      # repr_total: the writer's wall time
            extra_names = {"repr_rounds": rep["n_rounds"], "repr_bytes": rep["bytes"]}
            extra_names.update(n_read_names=sites.n_read_names)
            ms.update(infer=(t1 - t0) * 1e3, fetch=(t2 - t1) * 1e3 if csv is None else 0.0,
                      csv_write=(t3 - (t2 if csv is None else t1)) * 1e3)        # csv_write: the writer's wall time
            extra = {"csv_writer": "host"}
            if csv is not None:              # the device writer's own phases; they overlap, so they need not add up to csv_write
                ms.update(csv_format=csv["ms_format"], csv_copy=csv["ms_copy"], csv_pwrite=csv["ms_write"])
                extra = {"csv_writer": "device", "csv_text_bytes": csv["site_bytes"] + csv["indiv_bytes"], "csv_rounds": csv["n_rounds"]}
            if compress and csv is not None:     # the deflate kernels' time; file bytes, header blocks and markers included
                ms.update(csv_deflate=csv["ms_deflate"])
                extra.update(csv_compressed_bytes=csv["site_compressed"] + csv["indiv_compressed"], csv_stored_blocks=csv["n_stored"])
                if "n_by_type" in csv:           # level 2 ran on the device; header blocks are counted
                    extra.update(csv_fixed_blocks=csv["n_by_type"][1], csv_dynamic_blocks=csv["n_by_type"][2])
            elif compress:                       # the host route: zlib; its time is part of csv_write and it counts no stored blocks
                ms.update(csv_deflate=0.0)
                extra.update(csv_compressed_bytes=host_gz, csv_stored_blocks=None)
            print("M6A_TIMES " + json.dumps({"ms": ms, "d2h_bytes": d2h, "n_sites": sites.n_sites, "n_reads": sites.n_reads, **extra, **extra_names,
                                                "n_windows": sites.n_windows, "window_bytes": sites.window_bytes,
                                                "peak_bytes": sites.peak_bytes, "inflate": sites.ms_inflate,
                                                "compressed_bytes": sites.compressed_bytes, "n_bgzf_blocks": sites.n_bgzf_blocks,
                                                "stream_bytes": sites.stream_bytes, "n_streams": sites.n_streams,
                                                **({"n_replicates": sites.n_replicates} if sites.n_replicates > 1 else {})}), flush=True)
    finally:
        sites.close()
        engine.close()
