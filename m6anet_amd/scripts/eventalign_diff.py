"""`eventalign_diff` sub-command: two conditions' eventalign files -> each condition's two CSV files and OUT/data.diff.csv, the per-site
rank-sum test between them (include/m6a.h: m6a_site_ranksum).  Each condition is built and scored as `eventalign_inference` builds
and scores it (several files are pooled as replicates; BGZF, `-` and FIFOs are what the handle takes), as a job of its own with the
same --seed, and both handles stay open: the two site tables are joined on the host, the pair indices go up, the kernel compares the
two read_prob arrays where they lie, and 24 bytes per pair come back (gt, eq, z).  OUT/a and OUT/b hold what `eventalign_inference`
writes for the condition, byte for byte.
With --signal one more launch follows (include/m6a.h: m6a_site_signal_ranksum): the same test on each of the nine columns of the two
handles' X -- dwell_time, norm_std and norm_mean at positions -1, 0, +1 -- with the same pair indices, 288 bytes per pair come back,
and OUT/data.diff_signal.csv holds nine rows per shared site, in data.diff.csv's order of sites and X's order of columns.  Its q_value is
Benjamini-Hochberg over all rows of that file, nine tests per site in one family.  Every other file keeps its bytes.
With --ks the two-sample Kolmogorov-Smirnov test and the medians follow the rank-sum launch (include/m6a.h: m6a_site_ks) with the same
pair indices on the two read_prob arrays: 32 bytes per pair come back (d_pos, d_neg, med_a, med_b) and OUT/data.diff_ks.csv holds
median_a, median_b, median_shift = median_a - median_b, ks_d, ks_sign, p_value and q_value per shared site.  p_value is the Kolmogorov
limit distribution at sqrt(n m / (n + m)) D, conservative for small bags.  With --signal --ks m6a_site_signal_ks also runs on the two
X and OUT/data.diff_signal_ks.csv holds nine rows per site, one Benjamini-Hochberg family, its medians in the normalised units of X
(their conversion to pA is not built).  Every other file keeps its bytes.
With --ks --ks_exact one more launch follows each of the two (include/m6a.h: m6a_ks_exact): the host forms h = max(d_pos, d_neg) from
what has come back, (n, m, h) go up -- 24 bytes per test, nine tests per site under --signal -- and the exact finite-sample p-value,
scipy.stats.ks_2samp's, comes back, 8 bytes per test.  In both KS files p_value is then the exact value wherever the test is defined
(both bags non-empty and without NaN, the shorter at most 2047 reads, n m at most 10^8) and the limit's value elsewhere, q_value is
Benjamini-Hochberg over p_value as written, and a last column p_method says `exact` or `asymptotic`.  Every other file keeps its bytes,
and without --ks_exact so do these two."""
import os
import pathlib
import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

from . import dataprep, eventalign_inference, inference

# eventalign_inference.argparser()'s flags without --eventalign: a condition is scored whole, so --drop_unflushed_tail has no place
INFERENCE_FLAGS = tuple(f for f in eventalign_inference.INFERENCE_FLAGS if f != "--drop_unflushed_tail")


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    for side, what in (("a", "first"), ("b", "second")):
        parser.add_argument("--eventalign_" + side, required=True, nargs="+",
                            help="eventalign file(s) of the %s condition, each as `eventalign_inference --eventalign` takes it (plain text or "
                                 "BGZF, `-` for the standard input, a FIFO); several files are replicates and are pooled." % what)
    parser.add_argument("--out_dir", required=True,
                        help="directory for the results: a/ and b/ (the two CSV files of each condition) and data.diff.csv.")
    eventalign_inference._copy(dataprep.argparser(), parser, eventalign_inference.DATAPREP_FLAGS)
    eventalign_inference._copy(inference.argparser(), parser, INFERENCE_FLAGS)
    parser.add_argument("--window_mb", type=int, default=0,
                        help="parse each eventalign file in windows of this many MB, as `eventalign_inference --window_mb` does (0: resident).")
    parser.add_argument("--signal", action="store_true",
                        help="also write data.diff_signal.csv: the rank-sum test on each of the nine signal features of a shared site "
                             "(dwell_time, norm_std, norm_mean at positions -1, 0, +1), the model-free comparison.  Nine rows per site; "
                             "q_value is Benjamini-Hochberg over all rows of that file, nine tests per site in one family.")
    parser.add_argument("--ks", action="store_true",
                        help="also write data.diff_ks.csv: per shared site the medians of the two conditions' read probabilities, their "
                             "difference median_a - median_b, and the two-sample Kolmogorov-Smirnov statistic with its sign, the p-value of "
                             "the Kolmogorov limit distribution (conservative for small bags; --ks_exact gives scipy.stats.ks_2samp's exact p "
                             "instead) and its Benjamini-Hochberg q_value.  With --signal also data.diff_signal_ks.csv: the same on each of the "
                             "nine signal features, medians in normalised units, nine rows per site in one family.")
    parser.add_argument("--ks_exact", action="store_true",
                        help="with --ks: p_value in data.diff_ks.csv and data.diff_signal_ks.csv is the exact finite-sample p-value of the "
                             "Kolmogorov-Smirnov statistic, what scipy.stats.ks_2samp(method='exact') returns, wherever the shorter bag has at "
                             "most 2047 reads and the product of the two sizes is at most 10^8, and the limit distribution's elsewhere; "
                             "q_value corrects p_value as written and a last column p_method says `exact` or `asymptotic`.")
    return inference.add_site_proba(parser)


def argument_error(args):
    """the sentence for what is refused before anything is opened or a GPU is touched, or None"""
    a, b = list(args.eventalign_a), list(args.eventalign_b)
    if (a + b).count("-") > 1:
        return "`-` is the standard input and can be read once: it is given %d times" % (a + b).count("-")
    if args.num_iterations < 1:
        return "--num_iterations must be 1 or more, not %d" % args.num_iterations
    if args.batch_size < 1 or args.save_per_batch < 1:
        return "--batch_size and --save_per_batch must be 1 or more"
    if args.window_mb < 0:
        return "--window_mb must be 0 or more, not %d" % args.window_mb
    if not 0 <= int(args.seed) <= 0xffffffff:
        return "--seed must be between 0 and 2**32 - 1"
    if args.readcount_min < 1 or args.readcount_max < args.readcount_min:
        return "--readcount_min must be 1 or more and at most --readcount_max"
    if args.ks_exact and not args.ks:
        return "--ks_exact chooses the p-value of --ks and needs it"
    if str(args.device).lower().startswith("cpu"):
        return "--device cpu: this build runs the hot path on an MI355X only (no CPU fallback)"
    return None


def score(engine, sites, out_dir, args):
    """One condition as `eventalign_inference` scores and writes it (host writer); returns (site_prob, mod_ratio) of its sites."""
    from .. import _io
    from ..constants import DEFAULT_MIN_READS, N_SAMPLES
    pathlib.Path(out_dir).mkdir(parents=True, exist_ok=True)
    writer = sites.writer()
    try:
        if sites.n_sites == 0:               # what `eventalign_inference` leaves behind: the two header lines, then the loader's error
            writer.write_csv(out_dir, [], [], [], write_header=True, n_threads=args.n_processes)
            raise _io.M6AIOError("m6a_io error -4: no site with at least %d reads" % DEFAULT_MIN_READS, -4)
        i = sites.info
        engine.set_host_offsets(sites.off)
        engine.infer_ptrs(i.X, i.site_kmers, i.off, sites.n_sites, args.num_iterations, N_SAMPLES, args.read_proba_threshold, args.seed,
                          args.batch_size, args.save_per_batch, i.read_prob, i.site_prob, i.mod_ratio)
        engine.sync()
        read_prob, site_prob, mod_ratio = sites.fetch()
        writer.write_csv(out_dir, read_prob, site_prob, mod_ratio, write_header=True, n_threads=args.n_processes)
    finally:
        writer.close()
    return site_prob, mod_ratio


def compare(engine, sites_a, sites_b, pair_a, pair_b):
    """m6a_site_ranksum on the two handles' device arrays: the pair indices go up, (gt, eq, z) come back"""
    import numpy as np
    import torch
    P = int(pair_a.size)
    if P == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)
    dev = "cuda:%d" % engine.device
    ia, ib = torch.from_numpy(pair_a).to(dev), torch.from_numpy(pair_b).to(dev)      # pageable memory: the copies are done on return
    gt, eq = torch.empty(P, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.int64, device=dev)
    z = torch.empty(P, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(engine.device)
    a, b = sites_a.info, sites_b.info
    engine.site_ranksum_ptrs(a.read_prob, a.off, sites_a.n_sites, b.read_prob, b.off, sites_b.n_sites, ia.data_ptr(), ib.data_ptr(), P,
                             gt.data_ptr(), eq.data_ptr(), None, z.data_ptr())
    engine.sync()
    return gt.cpu().numpy(), eq.cpu().numpy(), z.cpu().numpy()


def compare_signal(engine, sites_a, sites_b, pair_a, pair_b):
    """m6a_site_signal_ranksum on the two handles' X where they lie: the pair indices go up, (gt, eq, z) [P, 9] come back"""
    import numpy as np
    import torch
    P = int(pair_a.size)
    if P == 0:
        return np.zeros((0, 9), np.int64), np.zeros((0, 9), np.int64), np.zeros((0, 9), np.float64)
    dev = "cuda:%d" % engine.device
    ia, ib = torch.from_numpy(pair_a).to(dev), torch.from_numpy(pair_b).to(dev)      # pageable memory: the copies are done on return
    gt, eq = torch.empty((P, 9), dtype=torch.int64, device=dev), torch.empty((P, 9), dtype=torch.int64, device=dev)
    z = torch.empty((P, 9), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(engine.device)
    a, b = sites_a.info, sites_b.info
    engine.site_signal_ranksum_ptrs(a.X, a.off, sites_a.n_sites, b.X, b.off, sites_b.n_sites, ia.data_ptr(), ib.data_ptr(), P,
                                    gt.data_ptr(), eq.data_ptr(), None, z.data_ptr())
    engine.sync()
    return gt.cpu().numpy(), eq.cpu().numpy(), z.cpu().numpy()


def compare_ks(engine, sites_a, sites_b, pair_a, pair_b, signal=False):
    """m6a_site_ks on the two handles' read_prob (signal: m6a_site_signal_ks on their X) where they lie: the pair indices go up,
    (d_pos, d_neg, med_a, med_b), each [P] or [P, 9], come back"""
    import numpy as np
    import torch
    P = int(pair_a.size)
    shape = (P, 9) if signal else (P,)
    if P == 0:
        return (np.zeros(shape, np.int64),) * 2 + (np.zeros(shape, np.float64),) * 2
    dev = "cuda:%d" % engine.device
    ia, ib = torch.from_numpy(pair_a).to(dev), torch.from_numpy(pair_b).to(dev)      # pageable memory: the copies are done on return
    out = [torch.empty(shape, dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.float64, torch.float64)]
    torch.cuda.synchronize(engine.device)
    a, b = sites_a.info, sites_b.info
    if signal:
        engine.site_signal_ks_ptrs(a.X, a.off, sites_a.n_sites, b.X, b.off, sites_b.n_sites, ia.data_ptr(), ib.data_ptr(), P,
                                   *[o.data_ptr() for o in out])
    else:
        engine.site_ks_ptrs(a.read_prob, a.off, sites_a.n_sites, b.read_prob, b.off, sites_b.n_sites, ia.data_ptr(), ib.data_ptr(), P,
                            *[o.data_ptr() for o in out])
    engine.sync()
    return tuple(o.cpu().numpy() for o in out)


def exact_p(engine, n_a, n_b, d_pos, d_neg):
    """m6a_ks_exact on what compare_ks brought back: the host forms h = max(d_pos, d_neg), (n, m, h) go up -- 24 bytes per test, the
    bag sizes repeated for the nine columns of a signal pair -- and p, of d_pos's shape, comes back; NaN where the test is undefined"""
    import numpy as np
    import torch

    from .. import ranksum
    h = ranksum.ks_h(d_pos, d_neg)
    if h.size == 0:
        return np.zeros(h.shape, np.float64)
    per_pair = h.size // int(np.size(n_a))                          # 1, or the nine columns
    dev = "cuda:%d" % engine.device
    up = [torch.from_numpy(np.ascontiguousarray(x, np.int64)).to(dev)
          for x in (np.repeat(np.asarray(n_a).ravel(), per_pair), np.repeat(np.asarray(n_b).ravel(), per_pair), h.ravel())]
    p = torch.empty(h.size, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(engine.device)
    engine.ks_exact_ptrs(*[x.data_ptr() for x in up], h.size, p.data_ptr())
    engine.sync()
    return p.cpu().numpy().reshape(h.shape)


def main(args):
    import threading

    import numpy as np

    from .. import _io, ranksum
    from ..data_utils import load_norm_factors

    text = argument_error(args)
    if text:
        print("m6anet_amd eventalign_diff: error: " + text, file=sys.stderr)
        raise SystemExit(2)
    weights = inference.resolve_model(args)
    device = inference._device_index(args.device)
    made = {}

    def make_engine():                       # the GPU context comes up while the first condition is parsed
        try:
            made["engine"] = inference.make_engine_for(args, weights, device)
        except BaseException as exc:        # re-raised on the main thread below
            made["error"] = exc

    def build(paths):                        # one file is a path, several are replicates: as --eventalign has them
        return _io.prep_sites(paths[0] if len(paths) == 1 else list(paths), args.readcount_min, args.readcount_max, args.min_segment_count,
                              load_norm_factors(args.norm_path), args.n_processes, device,
                              window_kb=args.window_mb * 1024 if args.window_mb else None)

    starter = threading.Thread(target=make_engine)
    starter.start()
    sites = []
    try:
        try:
            sites.append(build(args.eventalign_a))
        finally:
            starter.join()
        if "error" in made:
            raise made["error"]
        sites.append(build(args.eventalign_b))
        engine = made["engine"]
        sa, sb = sites
        site_a, mod_a = score(engine, sa, os.path.join(args.out_dir, "a"), args)
        site_b, mod_b = score(engine, sb, os.path.join(args.out_dir, "b"), args)
        names_a, names_b = np.asarray(sa.names, object), np.asarray(sb.names, object)
        pair_a, pair_b = ranksum.join(names_a[sa.site_tx], sa.tx_pos, names_b[sb.site_tx], sb.tx_pos)
        gt, eq, z = compare(engine, sa, sb, pair_a, pair_b)
        kmer = [bytes(k).decode() for k in sa.kmer7[pair_a, 1:6]]
        text = ranksum.diff_text(names_a[sa.site_tx[pair_a]], sa.tx_pos[pair_a], kmer, np.diff(sa.off)[pair_a], np.diff(sb.off)[pair_b],
                                 site_a[pair_a], site_b[pair_b], mod_a[pair_a], mod_b[pair_b], gt, eq, z)
        with open(os.path.join(args.out_dir, ranksum.DIFF_FILE), "w") as f:
            f.write(text)
        if args.ks:
            ks = compare_ks(engine, sa, sb, pair_a, pair_b)
            exact = {"p_exact": exact_p(engine, np.diff(sa.off)[pair_a], np.diff(sb.off)[pair_b], ks[0], ks[1])} if args.ks_exact else {}
            text = ranksum.ks_text(names_a[sa.site_tx[pair_a]], sa.tx_pos[pair_a], kmer, np.diff(sa.off)[pair_a], np.diff(sb.off)[pair_b],
                                   *ks, **exact)
            with open(os.path.join(args.out_dir, ranksum.KS_FILE), "w") as f:
                f.write(text)
        if args.signal:
            gt, eq, z = compare_signal(engine, sa, sb, pair_a, pair_b)
            text = ranksum.signal_text(names_a[sa.site_tx[pair_a]], sa.tx_pos[pair_a], kmer, np.diff(sa.off)[pair_a], np.diff(sb.off)[pair_b],
                                       gt, eq, z)
            with open(os.path.join(args.out_dir, ranksum.SIGNAL_FILE), "w") as f:
                f.write(text)
            if args.ks:
                ks = compare_ks(engine, sa, sb, pair_a, pair_b, signal=True)
                exact = {"p_exact": exact_p(engine, np.diff(sa.off)[pair_a], np.diff(sb.off)[pair_b], ks[0], ks[1])} if args.ks_exact else {}
                text = ranksum.signal_ks_text(names_a[sa.site_tx[pair_a]], sa.tx_pos[pair_a], kmer, np.diff(sa.off)[pair_a],
                                              np.diff(sb.off)[pair_b], *ks, **exact)
                with open(os.path.join(args.out_dir, ranksum.SIGNAL_KS_FILE), "w") as f:
                    f.write(text)
        print("eventalign_diff: %d sites in both conditions, %d only in A, %d only in B"
              % (pair_a.size, sa.n_sites - pair_a.size, sb.n_sites - np.unique(pair_b).size), flush=True)
    finally:
        for s in sites:
            s.close()
        if "engine" in made:
            made["engine"].close()
