"""`python -m m6anet_amd {dataprep,pack,inference,eventalign_inference,eventalign_diff,bgzip,train,compute_norm_factors} ...` -- the hot path and the steps before it
(dispatcher shape of m6anet/__init__.py:11-30)."""
import sys

from . import _early

if __name__ == "__main__":
    _early.maybe_start(sys.argv[1:])        # `inference --gpus N`: the other ranks start before the heavy imports below

from argparse import ArgumentParser  # noqa: E402

from .scripts import bgzip, compute_norm_factors, dataprep, eventalign_diff, eventalign_inference, inference, pack, train  # noqa: E402


def main(argv=None):
    parser = ArgumentParser(prog="m6anet_amd")
    sub = parser.add_subparsers(dest="command", required=True)
    sub.add_parser("inference", parents=[inference.full_parser()], help="run the MI355X inference hot path")
    sub.add_parser("dataprep", parents=[dataprep.argparser()], help="eventalign.txt -> data.json / data.info (native, host-only)")
    sub.add_parser("pack", parents=[pack.argparser()], help="data.json / data.info -> one binary site store that later runs map")
    sub.add_parser("eventalign_inference", parents=[eventalign_inference.grouped_parser()],
                   help="eventalign.txt -> the two CSVs in one process, the features kept in HBM (= dataprep, then inference)")
    sub.add_parser("eventalign_diff", parents=[eventalign_diff.argparser()],
                   help="two conditions' eventalign files -> each one's CSVs and data.diff.csv, the per-site rank-sum test between them")
    sub.add_parser("bgzip", parents=[bgzip.argparser()], help="FILE -> FILE.gz in BGZF, which eventalign_inference reads directly")
    sub.add_parser("train", parents=[train.argparser()], description=train.DESCRIPTION,
                   help="fit the model: training-mode forward, backward pass and Adam in HIP, the data set loaded once")
    sub.add_parser("compute_norm_factors", parents=[compute_norm_factors.argparser()],
                   help="data.json + data.info.labelled -> the per-5-mer mean and std that train and inference normalise with")
    args = parser.parse_args(argv)
    {"inference": inference, "dataprep": dataprep, "pack": pack, "eventalign_inference": eventalign_inference, "eventalign_diff": eventalign_diff,
     "bgzip": bgzip, "train": train, "compute_norm_factors": compute_norm_factors}[args.command].main(args)


if __name__ == "__main__":
    main(sys.argv[1:])
