"""Child process of tests/test_gpu_csv_device.py: every GPU step of that file runs here (or in the command itself), under
`timeout -k 10`, so that a hang or a fault ends with the child.

    python csv_device_child.py format JOB.pkl OUT.pkl      JOB: a list of (arrays, [(site_begin, site_end), ...]); OUT: per job and
                                                           range what _io.csv_format returned
    python csv_device_child.py declined EVENTALIGN OUT_DIR OUT.pkl
                                                           prep_sites(EVENTALIGN).write_csv(OUT_DIR) without inference: OUT holds the
                                                           exception's class name, code and n_declined (or "written")
    python csv_device_child.py append EVENTALIGN HOST_DIR PLAIN_DIR GZ1_DIR GZ2_DIR OUT.pkl
                                                           prep_sites + inference; the host writer into HOST_DIR, then on the one handle
                                                           write_csv(write_header=True) and write_csv(write_header=False) into PLAIN_DIR,
                                                           with compress=True into GZ1_DIR and at level 2 into GZ2_DIR; OUT: the statistics"""
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    from m6anet_amd import _io
    mode = sys.argv[1]
    if mode == "format":
        jobs = pickle.load(open(sys.argv[2], "rb"))
        out = []
        for a, ranges in jobs:
            out.append([_io.csv_format(a["off"], a["tx_pos"], a["tx_blob"], a["tx_off"], a["site_tx"], a["kmer5"], a["read_ids"], a["read_prob"],
                                       a["site_prob"], a["mod_ratio"], a.get("read_rep"), a.get("n_rep", 1), site_begin=b, site_end=e)
                        for b, e in ranges])
        pickle.dump(out, open(sys.argv[3], "wb"))
    elif mode == "declined":
        with _io.prep_sites(sys.argv[2], n_threads=4) as p:
            res = {"n_sites": p.n_sites, "ids_max": float(p.read_ids.max()) if p.n_reads else None, "d2h_before": p.times()[1]}
            try:
                p.write_csv(sys.argv[3], write_header=True, n_threads=2)
                res["what"] = "written"
            except _io.M6AIOError as e:
                res.update(what=type(e).__name__, code=e.code, n_declined=getattr(e, "n_declined", None), text=str(e))
            res["d2h_after"] = p.times()[1]
        pickle.dump(res, open(sys.argv[4], "wb"))
    elif mode == "append":
        from deflate_device_child import sites_with_outputs
        p, eng = sites_with_outputs([sys.argv[2]])
        res = {"n_sites": p.n_sites}
        p.writer().write_csv(sys.argv[3], *p.fetch(), write_header=True, n_threads=2)
        for key, out, kw in (("plain", sys.argv[4], {}), ("gz1", sys.argv[5], {"compress": True}), ("gz2", sys.argv[6], {"compress": True, "level": 2})):
            res[key] = [p.write_csv(out, write_header=h, n_threads=2, **kw) for h in (True, False)]
        p.close()
        eng.close()
        pickle.dump(res, open(sys.argv[7], "wb"))
    else:
        raise SystemExit("unknown mode %r" % mode)


if __name__ == "__main__":
    main()
