"""`inference` sub-command: same flags, defaults and output files as `m6anet inference`
(m6anet/scripts/inference.py:20-106), running the hot path on an MI355X through libm6a_hip.so."""
import os
import pathlib
import warnings
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

from ..constants import (DEFAULT_MIN_READS, DEFAULT_PRETRAINED_MODEL, DEFAULT_PRETRAINED_MODELS,
                         DEFAULT_READ_THRESHOLD, N_REPR, N_WEIGHT_FLOATS, PRETRAINED_CONFIGS)
from ..data_utils import STORE_SUFFIX, load_sites, load_sites_native, open_store
from ..engine import M6ANetEngine, load_weights, weights_from_state_dict
from ..inference_utils import INDIV_HEADER, SITE_HEADER, run_inference


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    parser.add_argument("--input_dir", nargs="*", required=True,
                        help="directories containing data.info and data.json, or ONE binary site store written by "
                             "`m6anet_amd pack` (*%s)." % STORE_SUFFIX)
    parser.add_argument("--out_dir", required=True, help="directory to output inference results.")
    parser.add_argument("--pretrained_model", default=DEFAULT_PRETRAINED_MODEL, type=str,
                        help="pre-trained model available at m6anet. Options include {}.".format(DEFAULT_PRETRAINED_MODELS))
    parser.add_argument("--model_config", default=None,
                        help="accepted for compatibility; only the m6anet.toml topology is supported.")
    parser.add_argument("--model_state_dict", default=None,
                        help="path to model weights: a reference .pt checkpoint (needs torch) or a flat .bin blob.")
    parser.add_argument("--norm_path", default=PRETRAINED_CONFIGS[DEFAULT_PRETRAINED_MODEL][2],
                        help="path to normalization factors file (.npz of this package or the reference's .joblib)")
    parser.add_argument("--batch_size", default=16, type=int, help="batch size for inference.")
    parser.add_argument("--save_per_batch", default=2, type=int,
                        help="saving inference results every save_per_batch multiples.")
    parser.add_argument("--n_processes", default=25, type=int,
                        help="accepted for compatibility; results are those of the reference at n_processes=1.")
    parser.add_argument("--num_iterations", default=1000, type=int, help="number of sampling run.")
    parser.add_argument("--device", default="cuda:0", type=str,
                        help="GPU to run on (cuda:N / hip:N). There is no CPU path.")
    parser.add_argument("--seed", default=0, type=int, help="random seed for sampling.")
    parser.add_argument("--read_proba_threshold", default=DEFAULT_READ_THRESHOLD, type=float,
                        help="default probability threshold for a read to be considered modified.")
    parser.add_argument("--gpus", default=1, type=int,
                        help="GPUs of this node to split the job's sites over: one process per GPU, flush-group-aligned shards, "
                             "every rank writes the rows of its own sites; the output does not depend on it.")
    parser.add_argument("--encoder", default=None, choices=["reference", "fast"],
                        help="read encoder kernel.  reference (the default, and the library's own default): the 16-slot kernels, which "
                             "perform the reference's float32 operations in the reference's order all the way to the sigmoid -- on the "
                             "host configuration it was validated against (torch + MKL on AVX-512) read probabilities are bit-identical "
                             "to `m6anet inference` wherever MKL groups a batch's rows in fours (every read of 20-read bags, > 99.9 %% "
                             "of ragged ones); activations beyond 2^64 saturate and a -inf pre-activation becomes NaN (DESIGN.md).  "
                             "fast: opt-in, for jobs whose bags all have >= 16 reads a 12-slot kernel 4-5 %% faster per step and within "
                             "rtol 1e-5 of the reference on every fixture (random fuzz: a few reads in 10^10 beyond that bar, worst 1.08 x).  "
                             "The encoder is under 1 %% of this command's wall time either way.  Without this flag the environment "
                             "variable M6A_ENCODER (auto|reference|general16|csite12|walk16|fast), if set, decides; an unknown value is an error.")
    parser.add_argument("--drop_unflushed_tail", action="store_true",
                        help="reference-compatible output: omit the batches after the reference's last flush, which "
                             "`m6anet inference` never writes (its flush test is inverted); default: write every site.")
    return parser


REPR_FILE = "data.read_representation.npy"
REPR_PIECE_READS = 1 << 20                            # rows per engine call and per write: 128 MB of representation at a time


def cli_parser():
    """argparser() -- the flags `eventalign_inference` and the ranks of --gpus N copy from -- and the flag that is this command's own"""
    parser = argparser()
    parser.add_argument("--loader", choices=("host", "device"), default="host",
                        help="who parses data.json.  host: the loader's threads, X streamed to the GPU from host memory.  device: the file "
                             "goes up whole and HIP kernels parse it (m6a_json_sites_build), X never leaves device memory and only read ids "
                             "and probabilities come back; the bytes written are the same.  Sites the kernels decline (an exponent, NaN, "
                             "anything malformed) are parsed by the host loader's code, and its errors are reported as its own.  One "
                             "--input_dir, no site store, --gpus 1.")
    return parser


SITE_PROBA_MODES = ("sampled", "expected")            # M6ANetEngine.set_site_mode


def add_site_proba(parser):
    """--site_proba, which `inference` and `eventalign_inference` add on top of their cli_parser()"""
    parser.add_argument("--site_proba", choices=SITE_PROBA_MODES, default="sampled",
                        help="what probability_modified in data.site_proba.csv is.  sampled: the reference's Monte-Carlo estimate, its "
                             "random draws replayed to the bit.  expected: the quantity those draws estimate, in closed form -- "
                             "1 - mean(1 - p)^20 over the site's reads -- which is deterministic and does not depend on the flush groups or "
                             "on --gpus; with it --num_iterations and --seed have no effect.  Every other column and data.indiv_proba.csv "
                             "are the same in both modes.")
    return parser


def command_parser():
    """cli_parser() and --site_proba: what `inference` shares with the ranks of --gpus N"""
    return add_site_proba(cli_parser())


def full_parser():
    """command_parser() and --read_representation, which no rank ever sees: the parser of the `inference` command"""
    parser = command_parser()
    parser.add_argument("--read_representation", action="store_true",
                        help="also write OUT_DIR/%s: float32 [n_reads][32], the read encoder's output -- layer 2 after its ReLU, "
                             "what the reference's MILModel.get_read_representation returns, bit for bit -- one row per data row of "
                             "data.indiv_proba.csv, in its order (np.load(..., mmap_mode='r') reads it without loading it: 128 bytes per "
                             "read).  Both CSVs are the bytes of a run without the flag.  One GPU, host loader: an argument error with "
                             "--gpus N > 1 or --loader device." % REPR_FILE)
    add_representation_dtype(parser)
    return parser


def add_representation_dtype(parser):
    """--representation_dtype, which `inference` and `eventalign_inference` add beside their --read_representation"""
    from argparse import SUPPRESS
    parser.add_argument("--representation_dtype", choices=("float32", "float16"), default=SUPPRESS,     # absent unless given: the check below
                        help="with --read_representation: the type of %s, float32 unless given.  float16 is each float32 value rounded once to the nearest "
                             "IEEE binary16 (ties to even; above 65504 is inf; subnormals kept) in the kernel that computes it -- exactly "
                             "what numpy's .astype(np.float16) makes of the float32 file -- at 64 bytes per read instead of 128, in the "
                             "file and across the link.  Without --read_representation it is an argument error." % REPR_FILE)
    return parser


def check_representation_dtype(args, command):
    """--representation_dtype without --read_representation: an argument error, before anything is written or a GPU is touched"""
    if hasattr(args, "representation_dtype") and not getattr(args, "read_representation", False):
        import sys
        print("m6anet_amd %s: error: --representation_dtype %s needs --read_representation" % (command, args.representation_dtype), file=sys.stderr)
        raise SystemExit(2)


def check_loader(args):
    """--loader device: what it refuses, as an argument error before any rank is launched or any file is written"""
    if getattr(args, "loader", "host") != "device":
        return
    import sys
    why = None
    if len(args.input_dir) != 1:
        why = "--loader device takes one --input_dir (%d given): replicates are pooled by the host loader" % len(args.input_dir)
    elif str(args.input_dir[0]).endswith(STORE_SUFFIX):
        why = "--loader device parses data.json; %s is a site store, which --loader host maps" % args.input_dir[0]
    elif args.gpus > 1 or "M6A_RANK" in os.environ:
        why = "--loader device runs on one GPU (--gpus %d given)" % args.gpus
    if why:
        print("m6anet_amd inference: error: %s" % why, file=sys.stderr)
        raise SystemExit(2)


def check_read_representation(args):
    """--read_representation: what it refuses, as an argument error before any rank is launched, any file is written or a GPU is touched"""
    check_representation_dtype(args, "inference")
    if not getattr(args, "read_representation", False):
        return
    import sys
    why = None
    if args.gpus > 1 or "M6A_RANK" in os.environ:
        why = "--read_representation writes one file from one GPU (--gpus %d given)" % args.gpus
    elif getattr(args, "loader", "host") == "device":
        why = "--read_representation takes the host loader's arrays (--loader device given)"
    if why:
        print("m6anet_amd inference: error: %s" % why, file=sys.stderr)
        raise SystemExit(2)


def write_read_representation(engine, batch, args):
    """OUT_DIR/data.read_representation.npy, row i = data row i of data.indiv_proba.csv: pieces of whole sites go through
    engine.get_read_representation into one reused buffer and from there into the memory-mapped file, so the process never holds
    more than a piece of it.  --representation_dtype float16: the memmap and the buffer are float16 and the engine is asked for it."""
    import numpy as np
    name = getattr(args, "representation_dtype", "float32")
    dtype = np.dtype(name)
    n_sites = batch.n_sites
    if getattr(args, "drop_unflushed_tail", False):
        from ..engine import reference_written_sites
        n_sites = reference_written_sites(batch.n_sites, args.batch_size, args.save_per_batch)
    off = np.ascontiguousarray(batch.off, np.int64)
    n_rows = int(off[n_sites])
    if n_rows == 0:                                       # an empty file cannot be mapped
        np.save(os.path.join(args.out_dir, REPR_FILE), np.empty((0, N_REPR), dtype))
        return
    out = np.lib.format.open_memmap(os.path.join(args.out_dir, REPR_FILE), mode="w+", dtype=dtype, shape=(n_rows, N_REPR))
    widest = int(np.diff(off[:n_sites + 1]).max(initial=0))      # a bag larger than a piece is a piece of its own
    piece = np.empty((min(max(widest, REPR_PIECE_READS), n_rows), N_REPR), dtype)
    s0 = 0
    while s0 < n_sites:
        s1 = int(np.searchsorted(off, off[s0] + REPR_PIECE_READS, side="right")) - 1
        s1 = min(n_sites, max(s1, s0 + 1))
        r0, r1 = int(off[s0]), int(off[s1])
        if r1 > r0:
            engine.get_read_representation(batch.X[r0:r1], batch.site_kmers[s0:s1], off[s0:s1 + 1] - r0, out=piece[:r1 - r0],
                                           **({"dtype": name} if name != "float32" else {}))
            out[r0:r1] = piece[:r1 - r0]
        s0 = s1
    out.flush()
    del out


def load_on_device(args):
    """--loader device, step 1: data.json parsed in HBM (m6a_json_sites_build); the prep_sites that holds X there"""
    from .. import _io
    from ..data_utils import load_norm_factors
    return _io.json_sites(args.input_dir[0], DEFAULT_MIN_READS, load_norm_factors(args.norm_path), args.n_processes, _device_index(args.device))


def run_on_device_sites(engine, sites, args):
    """--loader device, the rest: inference on the handle's device pointers, 13 B per read back, the rows through the host writer
    under the headers main() wrote -- the bytes run_inference writes for the host loader's arrays."""
    from ..constants import N_SAMPLES
    from ..engine import reference_written_sites
    i = sites.info
    engine.set_host_offsets(sites.off)
    engine.infer_ptrs(i.X, i.site_kmers, i.off, sites.n_sites, args.num_iterations, N_SAMPLES, args.read_proba_threshold, args.seed,
                      args.batch_size, args.save_per_batch, i.read_prob, i.site_prob, i.mod_ratio)
    engine.sync()
    read_prob, site_prob, mod_ratio = sites.fetch()
    n_write = None
    if getattr(args, "drop_unflushed_tail", False):
        n_write = reference_written_sites(sites.n_sites, args.batch_size, args.save_per_batch)
    sites.writer().write_csv(args.out_dir, read_prob, site_prob, mod_ratio, write_header=False, n_threads=args.n_processes, n_sites=n_write)
    if os.environ.get("M6A_LOADER_TIMES"):               # phases for tools/measure_loader.py
        import json
        ms, d2h = sites.times()
        print("M6A_TIMES " + json.dumps({"ms": ms, "d2h_bytes": d2h, "n_sites": sites.n_sites, "n_reads": sites.n_reads,
                                            "n_declined_sites": sites.n_declined_sites, "peak_bytes": sites.peak_bytes}), flush=True)


ENCODER_MODES = {"reference": 1, "fast": 4}           # m6a_set_encoder_variant (include/m6a.h)
ENCODER_ENV_VALUES = ("", "auto", "reference", "general16", "csite12", "walk16", "fast")


def make_engine_for(args, weights, device):
    """The context of one `inference` process with --encoder applied to IT (m6a_set_encoder_variant), not to the process's
    environment: a library caller's other contexts keep their own choice.  An explicit --encoder always wins; without the
    flag M6A_ENCODER decides if set (m6a_create reads it and refuses values it does not know -- checked here first, so the
    message names the variable), else `reference`, which is also what the library does when nobody says anything."""
    env = os.environ.get("M6A_ENCODER")
    if env is not None and env not in ENCODER_ENV_VALUES:
        raise ValueError("M6A_ENCODER=%s: must be one of %s" % (env, "|".join(v for v in ENCODER_ENV_VALUES if v)))
    engine = M6ANetEngine(weights=weights, device=device)
    if getattr(args, "site_proba", "sampled") == "expected":     # first: the context's background set-up for the sampling stops
        engine.set_site_mode("expected")
    choice = getattr(args, "encoder", None)
    if choice is not None:
        engine.set_encoder_variant(ENCODER_MODES[choice])
    elif env is None:
        engine.set_encoder_variant(ENCODER_MODES["reference"])
    return engine


def _device_index(device):
    d = str(device).lower()
    if d.startswith("cpu"):
        raise ValueError("--device cpu: this build runs the hot path on an MI355X only (no CPU fallback)")
    return int(d.split(":")[1]) if ":" in d else 0


def _check_model_config(path):
    """Only the m6anet.toml topology exists here (m6anet/model/configs/model_configs/m6anet.toml); any other
    block list would silently run the wrong network."""
    import tomli
    with open(path, "rb") as f:
        blocks = tomli.load(f).get("block", [])
    want = ["DeaggregateNanopolish", "KmerMultipleEmbedding", "ConcatenateFeatures", "Linear", "Linear", "SigmoidProdPooling"]
    got = [b.get("block_type") for b in blocks]
    dims = [(b.get("input_channel"), b.get("output_channel")) for b in blocks if b.get("block_type") == "Linear"]
    if got != want or dims != [(15, 150), (150, 32)]:
        raise ValueError("--model_config %s is not the m6anet.toml topology (blocks %s): not supported" % (path, got))


def resolve_model(args):
    """The weights of this run; a pretrained model also sets args.read_proba_threshold and args.norm_path (the reference's rule)."""
    if not 0 <= int(args.seed) <= 0xffffffff:
        raise ValueError("Seed must be between 0 and 2**32 - 1")        # what np.random.seed raises
    if args.model_config is not None:
        _check_model_config(args.model_config)
    if args.model_state_dict is not None:
        warnings.warn("--model_state_dict is specified, overwriting default model weights")
        if str(args.model_state_dict).endswith(".bin"):
            import numpy as np
            weights = np.fromfile(args.model_state_dict, np.float32)
            if weights.size != N_WEIGHT_FLOATS:
                raise ValueError("%s holds %d floats, expected %d (layout in include/m6a.h)"
                                 % (args.model_state_dict, weights.size, N_WEIGHT_FLOATS))
        else:
            import torch
            weights = weights_from_state_dict(torch.load(args.model_state_dict, map_location="cpu", weights_only=True))
    else:
        if args.pretrained_model not in DEFAULT_PRETRAINED_MODELS:
            raise ValueError("Invalid pretrained model {}, must be one of {}".format(
                args.pretrained_model, DEFAULT_PRETRAINED_MODELS))
        weights = load_weights(args.pretrained_model)
        args.read_proba_threshold = PRETRAINED_CONFIGS[args.pretrained_model][1]
        args.norm_path = PRETRAINED_CONFIGS[args.pretrained_model][2]
    return weights


def main(args):
    check_loader(args)
    check_read_representation(args)
    weights = resolve_model(args)
    if args.gpus < 1:
        raise ValueError("--gpus must be >= 1")
    if "M6A_RANK" in os.environ:                         # one rank of a --gpus N job (started by multi_gpu.launch)
        from .. import multi_gpu
        multi_gpu.run_rank(args, weights)
        return
    if args.gpus > 1:
        from .. import multi_gpu
        pathlib.Path(args.out_dir).mkdir(parents=True, exist_ok=True)
        rc = multi_gpu.launch(args, weights)
        if rc != 0:
            raise SystemExit(rc)
        return

    # the GPU context (HIP initialisation, weights) comes up on a thread while the loader parses data.json
    import threading
    made = {}

    on_device = getattr(args, "loader", "host") == "device"

    def make_engine():
        try:
            made["engine"] = make_engine_for(args, weights, _device_index(args.device))
            if not on_device:
                made["engine"].prepare_host_io()     # pinned staging for the host arrays the loader is producing
        except BaseException as exc:        # re-raised on the main thread below
            made["error"] = exc

    starter = threading.Thread(target=make_engine)
    starter.start()
    pathlib.Path(args.out_dir).mkdir(parents=True, exist_ok=True)
    with open(os.path.join(args.out_dir, "data.site_proba.csv"), "w", encoding="utf-8") as f:
        f.write(SITE_HEADER)
    with open(os.path.join(args.out_dir, "data.indiv_proba.csv"), "w", encoding="utf-8") as g:
        g.write(INDIV_HEADER)
    if on_device:                            # data.json is parsed in HBM while the context comes up
        try:
            sites = load_on_device(args)
        except BaseException:
            starter.join()
            if "engine" in made:
                made["engine"].close()
            raise
        starter.join()
        try:
            if "error" in made:
                raise made["error"]
            run_on_device_sites(made["engine"], sites, args)
        finally:
            sites.close()
            if "engine" in made:
                made["engine"].close()
        return
    # --n_processes is the reference's host-parallelism flag: here it sizes the loader / writer threads
    if any(str(d).endswith(STORE_SUFFIX) for d in args.input_dir):
        if len(args.input_dir) != 1:
            raise ValueError("--input_dir takes ONE site store (pack replicates together with `m6anet_amd pack`)")
        batch = open_store(args.input_dir[0], args.norm_path, DEFAULT_MIN_READS)
    else:
        try:
            batch = load_sites_native(args.input_dir, DEFAULT_MIN_READS, args.norm_path, n_threads=args.n_processes)
        except ImportError:
            batch = load_sites(args.input_dir, DEFAULT_MIN_READS, args.norm_path)   # libm6a_io.so not built
    starter.join()
    if "error" in made:
        raise made["error"]
    engine = made["engine"]
    run_inference(engine, batch, args)
    if getattr(args, "read_representation", False):
        write_read_representation(engine, batch, args)
    engine.close()
