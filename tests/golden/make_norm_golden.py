#!/usr/bin/env python3
"""Generate tests/golden/norm_ref/ by CALLING the reference (the conventions of make_golden.py: its functions are called on its own
data and inputs / outputs are stored as data; nothing of its source is copied).

    python tests/golden/make_norm_golden.py

  data.info.labelled   the reference's own test file (its rows name the records of tests/golden/ref_tests_data/data.json)
  norm_factors.npz     kmers, mean [K][3], std [K][3]: what annotate_kmer_information, create_kmer_mapping_df and create_norm_dict of
                       m6anet/utils/norm_utils.py return on it with one process, as m6anet/scripts/compute_norm_factors.py calls them
The module is loaded by its file path: `import m6anet` pulls in packages this project does not need.
"""
import importlib.util
import os
import shutil
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("M6ANET_REFERENCE", "/root/reference")         # the reference checkout, as in make_golden.py
OUT = os.path.join(HERE, "norm_ref")

sys.dont_write_bytecode = True
spec = importlib.util.spec_from_file_location("ref_norm_utils", os.path.join(REF, "m6anet", "utils", "norm_utils.py"))
norm_utils = importlib.util.module_from_spec(spec)
sys.modules["ref_norm_utils"] = norm_utils                          # multiprocessing pickles its functions by module name
spec.loader.exec_module(norm_utils)


def main():
    data = os.path.join(REF, "m6anet", "tests", "data")
    os.makedirs(OUT, exist_ok=True)
    shutil.copyfile(os.path.join(data, "data.info.labelled"), os.path.join(OUT, "data.info.labelled"))
    with open(os.path.join(data, "data.json"), "rb") as f, open(os.path.join(HERE, "ref_tests_data", "data.json"), "rb") as g:
        assert f.read() == g.read(), "tests/golden/ref_tests_data/data.json is not the reference's"
    data_fpath = os.path.join(data, "data.json")
    info_df = pd.read_csv(os.path.join(data, "data.info.labelled"))
    info_df = info_df[info_df["set_type"] == "Train"].copy()
    info_df["transcript_position"] = info_df["transcript_position"].astype("int")
    info_df = norm_utils.annotate_kmer_information(data_fpath, info_df, 1)
    norm = norm_utils.create_norm_dict(norm_utils.create_kmer_mapping_df(info_df), data_fpath, 1)
    kmers = sorted(norm)
    np.savez(os.path.join(OUT, "norm_factors.npz"), kmers=np.array(kmers), mean=np.array([norm[k][0] for k in kmers], np.float64),
             std=np.array([norm[k][1] for k in kmers], np.float64))
    print("%d Train sites, %d 5-mers -> %s" % (len(info_df), len(kmers), OUT))


if __name__ == "__main__":
    main()
