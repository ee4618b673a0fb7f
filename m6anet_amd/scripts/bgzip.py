"""`bgzip` sub-command: FILE -> FILE.gz in BGZF (m6anet_amd/bgzf.py), the compressed form `eventalign_inference` reads directly, for
users without htslib.  Python's zlib, 0xff00 input bytes per block, then the end-of-file marker."""
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    parser.add_argument("file", metavar="FILE", help="the file to compress; FILE.gz is written beside it and FILE stays.")
    parser.add_argument("--level", type=int, default=6, choices=range(0, 10), metavar="N", help="zlib compression level, 0..9.")
    parser.add_argument("--n_processes", type=int, default=1, help="processes that compress spans of blocks.")
    return parser


def main(args):
    from .. import bgzf
    n_in, n_out = bgzf.compress_file(args.file, level=args.level, n_processes=max(1, args.n_processes))
    print("%s.gz: %d -> %d bytes (%.2fx)" % (args.file, n_in, n_out, n_in / max(1, n_out)))
