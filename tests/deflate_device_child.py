"""Child process of tests/test_gpu_deflate.py: every GPU step of that file runs here (or in the command itself), under
`timeout -k 10`, so that a hang or a fault ends with the child.

    python deflate_device_child.py deflate IN.pkl OUT.pkl WORK_DIR   IN: {name: text}; OUT: {name: (what _io.bgzf_deflate gave, its stats,
                                                                     whether _io.bgzf_inflate of a file of it returned the text)}
    python deflate_device_child.py write OUT.pkl PLAIN_DIR GZ_DIR EVENTALIGN...
                                                                     prep_sites + inference, then write_csv into PLAIN_DIR and
                                                                     write_csv(compress=True) into GZ_DIR; OUT: both statistics
    python deflate_device_child.py budget OUT.pkl GZ_DIR EVENTALIGN...
                                                                     the same up to inference; write_csv(compress=True) under
                                                                     M6A_PREP_BUDGET_MB=1, what it raised and what GZ_DIR held then, and
                                                                     the call again without the variable"""
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sites_with_outputs(files):
    from m6anet_amd import _io
    from m6anet_amd.engine import M6ANetEngine, load_weights
    p = _io.prep_sites(files if len(files) > 1 else files[0], min_segment_count=1, n_threads=4)
    eng = M6ANetEngine(weights=load_weights("HCT116_RNA002"), device=0)
    i = p.info
    eng.set_host_offsets(p.off)
    eng.infer_ptrs(i.X, i.site_kmers, i.off, p.n_sites, 20, read_prob=i.read_prob, site_prob=i.site_prob, mod_ratio=i.mod_ratio)
    eng.sync()
    return p, eng


def main():
    from m6anet_amd import _io
    mode = sys.argv[1]
    if mode == "deflate":
        texts = pickle.load(open(sys.argv[2], "rb"))
        path, out = os.path.join(sys.argv[4], "device.gz"), {}
        for name, text in texts.items():
            st = {}
            data = _io.bgzf_deflate(text, stats=st)
            with open(path, "wb") as f:
                f.write(data)
            out[name] = (data, st, _io.bgzf_inflate(path) == text)
        pickle.dump(out, open(sys.argv[3], "wb"))
    elif mode == "write":
        p, eng = sites_with_outputs(sys.argv[5:])
        res = {"n_sites": p.n_sites, "plain": p.write_csv(sys.argv[3], write_header=True, n_threads=2)}
        before = p.times()[1]
        res["gz"] = p.write_csv(sys.argv[4], write_header=True, n_threads=2, compress=True)
        res["d2h_grew"] = p.times()[1] - before
        res["peak_bytes"] = p.peak_bytes
        p.close()
        eng.close()
        pickle.dump(res, open(sys.argv[2], "wb"))
    elif mode == "budget":
        p, eng = sites_with_outputs(sys.argv[4:])
        res = {}
        os.environ["M6A_PREP_BUDGET_MB"] = "1"
        try:
            p.write_csv(sys.argv[3], write_header=True, n_threads=2, compress=True)
            res["what"] = "written"
        except _io.M6AIOError as e:
            res.update(what=type(e).__name__, code=e.code, text=str(e))
        res["left"] = sorted(os.listdir(sys.argv[3]))
        del os.environ["M6A_PREP_BUDGET_MB"]
        res["gz"] = p.write_csv(sys.argv[3], write_header=True, n_threads=2, compress=True)
        p.close()
        eng.close()
        pickle.dump(res, open(sys.argv[2], "wb"))
    else:
        raise SystemExit("unknown mode %r" % mode)


if __name__ == "__main__":
    main()
