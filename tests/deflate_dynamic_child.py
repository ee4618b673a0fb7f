"""Child process of tests/test_gpu_deflate_dynamic.py: every GPU step of that file runs here (or in the command itself), under
`timeout -k 10`, so that a hang or a fault ends with the child.

    python deflate_dynamic_child.py deflate IN.pkl OUT.pkl WORK_DIR  IN: {name: text}; OUT: {name: (what _io.bgzf_deflate(level=2) gave,
                                                                     its stats, whether _io.bgzf_inflate of a file of it returned the
                                                                     text, whether level=1 through m6a_bgzf_deflate_level gave
                                                                     _io.bgzf_deflate's bytes)}
    python deflate_dynamic_child.py write OUT.pkl PLAIN_DIR GZ1_DIR GZ2_DIR EVENTALIGN...
                                                                     prep_sites + inference, then write_csv into PLAIN_DIR,
                                                                     write_csv(compress=True) into GZ1_DIR and
                                                                     write_csv(compress=True, level=2) into GZ2_DIR; OUT: the statistics"""
import ctypes as C
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def level_1_through_the_new_symbol(text):
    from m6anet_amd import _lib
    L, n, st, by = _lib.load(), C.c_int64(), _lib.DeflateStats(), (C.c_int64 * 3)()
    assert L.m6a_bgzf_deflate_level(0, text, len(text), 1, None, 0, C.byref(n), None, None) == 0
    buf = C.create_string_buffer(n.value)
    assert L.m6a_bgzf_deflate_level(0, text, len(text), 1, buf, n.value, C.byref(n), C.byref(st), by) == 0
    return buf.raw[:n.value], list(by)


def main():
    from m6anet_amd import _io
    mode = sys.argv[1]
    if mode == "deflate":
        texts = pickle.load(open(sys.argv[2], "rb"))
        path, out = os.path.join(sys.argv[4], "device.gz"), {}
        for name, text in texts.items():
            st, st1 = {}, {}
            data = _io.bgzf_deflate(text, stats=st, level=2)
            with open(path, "wb") as f:
                f.write(data)
            one, by = level_1_through_the_new_symbol(text)
            same = one == _io.bgzf_deflate(text, stats=st1) and by == [st1["n_stored"], st1["n_blocks"] - st1["n_stored"], 0]
            out[name] = (data, st, _io.bgzf_inflate(path) == text, same)
        pickle.dump(out, open(sys.argv[3], "wb"))
    elif mode == "write":
        from deflate_device_child import sites_with_outputs
        p, eng = sites_with_outputs(sys.argv[6:])
        res = {"n_sites": p.n_sites, "plain": p.write_csv(sys.argv[3], write_header=True, n_threads=2)}
        res["gz1"] = p.write_csv(sys.argv[4], write_header=True, n_threads=2, compress=True)
        before = p.times()[1]
        res["gz2"] = p.write_csv(sys.argv[5], write_header=True, n_threads=2, compress=True, level=2)
        res["d2h_grew"] = p.times()[1] - before
        p.close()
        eng.close()
        pickle.dump(res, open(sys.argv[2], "wb"))
    else:
        raise SystemExit("unknown mode %r" % mode)


if __name__ == "__main__":
    main()
