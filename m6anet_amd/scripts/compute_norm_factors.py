"""`compute_norm_factors` sub-command: the flags of `m6anet compute_norm_factors` (m6anet/scripts/compute_norm_factors.py:10-43) -- the
per-5-mer mean and std of the Train sites of data.info.labelled, the step between `dataprep` and `train` -- summed by HIP kernels on
an MI355X (include/m6a.h: m6a_norm_factors_build) or, with --device cpu, by libm6a_io.so; the reference's bits either way."""
import json
import os
import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

OUT_STEM = "norm_dict_nanopolish"


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    parser.add_argument("--input_dir", required=True, help="Input directory containing the data.info.labelled file and data.json file")
    parser.add_argument("--out_dir", required=True, help="Output directory for the normalization file")
    parser.add_argument("--n_processes", default=1, type=int, help="threads that parse the sites the host handles.")
    parser.add_argument("--device", default="gpu", choices=("cpu", "gpu"),
                        help="gpu: parse data.json and sum in HIP on GPU 0 (data.json and 72 bytes per read must fit in device memory); "
                             "cpu: the same numbers from the host.")
    return parser


class Refusal(Exception):
    pass


def plan(args):
    """Everything that can be refused, decided before anything is written or a GPU is touched.  -> the site table."""
    from ..data_utils import read_norm_sites
    if args.n_processes < 1:
        raise Refusal("--n_processes must be >= 1")
    try:
        return read_norm_sites(args.input_dir)
    except (ValueError, OSError) as e:
        raise Refusal(str(e))


def main(args):
    import time
    t0 = time.perf_counter()
    try:
        tx, pos, start, end, n_reads = plan(args)
    except Refusal as e:
        print("m6anet_amd compute_norm_factors: error: %s" % e, file=sys.stderr)
        raise SystemExit(2)
    from .. import _io
    from ..data_utils import save_norm_factors
    t1 = time.perf_counter()
    r = _io.norm_factors(os.path.join(args.input_dir, "data.json"), tx, pos, start, end, n_reads,
                         device="cpu" if args.device == "cpu" else 0, n_threads=args.n_processes)
    t2 = time.perf_counter()
    os.makedirs(args.out_dir, exist_ok=True)
    paths = save_norm_factors(os.path.join(args.out_dir, OUT_STEM), {k: (r["mean"][i], r["std"][i]) for i, k in enumerate(r["kmers"])})
    t3 = time.perf_counter()
    print("%d Train sites, %d reads, %d 5-mers -> %s" % (len(tx), int(n_reads.sum()), len(r["kmers"]), ", ".join(paths)))
    if os.environ.get("M6A_NORM_TIMES"):
        st = r.get("stats", {})
        print("M6A_TIMES " + json.dumps({
            "device": args.device, "ms_labelled": (t1 - t0) * 1e3, "ms_factors": (t2 - t1) * 1e3, "ms_write": (t3 - t2) * 1e3,
            "ms_total": (t3 - t0) * 1e3, "ms_upload": st.get("ms_upload", 0.0), "ms_kernels": st.get("ms_kernels", 0.0),
            "ms_host_half": st.get("ms_host", 0.0), "ms_fold": st.get("ms_fold", 0.0), "n_sites": len(tx), "n_reads": int(n_reads.sum()),
            "n_kmers": len(r["kmers"]), "n_declined": int(st.get("n_declined", 0)), "d2h_bytes": int(st.get("d2h_bytes", 0)),
            "peak_device_bytes": int(st.get("peak_bytes", 0))}), file=sys.stderr)
