"""`eventalign_inference --read_names` on the device (include/m6a.h: m6a_prep_sites_build_names), held to its twin: a file whose
field 4 is the read's UUID gives the arrays of the same file with every name replaced by its dense index -- X bit for bit -- on the
families of tests/read_names_gen.py, whole, in windows, as BGZF and as replicates; the table of names is the statement's; the names
add 16 bytes each to the device-to-host traffic and nothing else; the command writes the twin's bytes with the UUID in column 3 of
data.indiv_proba.csv through the host writer, the device writer and both compressed forms; and what is no name is an error with the
statement's text and offset that leaves no CSV behind."""
import gzip
import os

import numpy as np
import pytest

import read_names_gen as NG
import read_names_statement as RS
from m6anet_amd import _io, bgzf
from test_eventalign_statement import hct116
from test_gpu_eventalign_inference import CSVS, run

pytestmark = pytest.mark.gpu


def arrays(p):
    X, km, off = p.inputs()
    return dict(X=X.view(np.uint32), km=km, off=off, off_host=p.off, site_tx=p.site_tx, tx_pos=p.tx_pos, kmer7=p.kmer7,
                read_ids=p.read_ids.view(np.uint64), read_rep=p.read_rep, tx_off=p.tx_off, blob=np.frombuffer(p.tx_blob, np.uint8))


def same(a, b, tag):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (tag, k)


def table_is(p, tables, tag):
    names, offsets = p.read_names
    assert offsets.tolist() == np.cumsum([0] + [len(t) for t in tables]).tolist(), tag
    assert names.dtype == np.uint8 and np.array_equal(names, np.concatenate([RS.table(t) for t in tables])), tag
    assert p.n_read_names == sum(len(t) for t in tables)


def twin_of(path, **kw):
    with _io.prep_sites(path, n_threads=2, **kw) as p:
        assert p.read_names is None and p.n_read_names == 0
        return arrays(p), p.n_sites, p.times()[1]


@pytest.mark.parametrize("family", NG.ARRAY_FAMILIES)
def test_named_file_equals_its_twin(tmp_path, family):
    c = NG.case(family)
    named, twin = c.write(tmp_path)
    for norm in (None, hct116()):
        want, n_sites, d2h_twin = twin_of(twin, norm=norm)
        assert n_sites > 0, family                                 # an equality over no sites shows nothing
        with _io.prep_sites(named, norm=norm, n_threads=2, read_names=True) as p:
            same(arrays(p), want, family)
            table_is(p, [c.names], family)
            assert p.n_sites == n_sites and p.read_ids.max() < len(c.names)
            d2h = p.times()[1]
        print("%s: %d names, d2h %d B named, %d B twin" % (family, len(c.names), d2h, d2h_twin))
        assert d2h - d2h_twin == 16 * len(c.names), family         # one copy of the table, and nothing else


@pytest.mark.parametrize("window_kb", NG.WINDOWS_KB)
def test_named_file_in_windows(tmp_path, window_kb):
    c = NG.case("windows")
    kinds = [k for *_, k in NG.cuts(c.named, window_kb << 10)]
    assert any("same_name" in k for k in kinds) and any("inside" in k for k in kinds)
    named, twin = c.write(tmp_path)
    want, n_sites, _ = twin_of(twin)
    assert n_sites > 0
    with _io.prep_sites(named, n_threads=2, read_names=True) as p:
        whole = arrays(p)
        table_is(p, [c.names], "whole")
    same(whole, want, "whole")
    with _io.prep_sites(named, n_threads=2, read_names=True, window_kb=window_kb) as p:
        same(arrays(p), whole, window_kb)
        table_is(p, [c.names], window_kb)
        assert p.n_windows == len(kinds) > 1, (p.n_windows, len(kinds))
    with _io.prep_sites(c.write(tmp_path)[0], n_threads=2, read_names=True, window_kb=window_kb, norm=hct116()) as p, \
            _io.prep_sites(twin, n_threads=2, norm=hct116()) as q:
        same(arrays(p), arrays(q), (window_kb, "norm"))


def test_named_bgzf_file(tmp_path):
    c = NG.case("again")
    named, twin = c.write(tmp_path)
    gz = tmp_path / "again_named.txt.gz"
    gz.write_bytes(bgzf.compress(c.named, block_input=3000))
    assert _io.is_bgzf(str(gz))
    want, n_sites, _ = twin_of(twin)
    with _io.prep_sites(str(gz), n_threads=2, read_names=True) as p:
        assert p.n_bgzf_blocks > 1 and p.n_sites == n_sites > 0
        same(arrays(p), want, "bgzf")
        table_is(p, [c.names], "bgzf")


@pytest.fixture(scope="module")
def replicate_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("named_replicates")
    reps = NG.replicates("split")
    paths = []
    for k, (named, twin, _) in enumerate(reps):
        paths.append((str(d / ("named_%d.txt" % k)), str(d / ("twin_%d.txt" % k))))
        open(paths[-1][0], "wb").write(named)
        open(paths[-1][1], "wb").write(twin)
    return [p[0] for p in paths], [p[1] for p in paths], [names for _, _, names in reps]


def test_named_replicates(replicate_files):
    named, twin, tables = replicate_files
    assert set(tables[0]) & set(tables[1]) and tables[1][0] == tables[0][3]      # a shared name has another index in each file
    want, n_sites, d2h_twin = twin_of(twin, norm=hct116(), min_segment_count=1)
    assert n_sites > 0
    with _io.prep_sites(named, norm=hct116(), n_threads=2, read_names=True, min_segment_count=1) as p:
        same(arrays(p), want, "replicates")
        table_is(p, tables, "replicates")
        assert p.n_replicates == 2 and p.times()[1] - d2h_twin == 16 * sum(map(len, tables))


# ---- the command ---------------------------------------------------------------------------------------------------------------------
MODES = {"host": ["--csv", "host"], "device": ["--csv", "device"], "gz1": ["--csv", "device", "--compress", "--compress_level", "1"],
         "gz2": ["--csv", "device", "--compress", "--compress_level", "2"]}
COMMON = ["--n_processes", "2", "--num_iterations", "50"]


def command_files(fixture, tmp_path_factory, replicate_files):
    """(named, twin, tables, flags)"""
    if fixture == "replicates":                                # parts of a site count from one read on, as where the fixture is pooled elsewhere
        return (*replicate_files, ["--min_segment_count", "1"])
    c = NG.case(fixture)
    named, twin = c.write(tmp_path_factory.mktemp("cmd_" + fixture))
    return named, twin, [c.names], []


def as_list(x):
    return list(x) if isinstance(x, list) else [x]


@pytest.fixture(scope="module")
def twin_texts(tmp_path_factory, replicate_files):
    """the twin command's two texts per fixture, written once (the host writer; its other writers are held to it elsewhere)"""
    made = {}

    def get(fixture):
        if fixture not in made:
            named, twin, tables, flags = command_files(fixture, tmp_path_factory, replicate_files)
            out = str(tmp_path_factory.mktemp("twin_out_" + fixture))
            run(["eventalign_inference", "--out_dir", out, "--eventalign"] + as_list(twin) + COMMON + flags, timeout=300)
            made[fixture] = (named, tables, flags, tuple(open(os.path.join(out, f), "rb").read() for f in CSVS))
        return made[fixture]
    return get


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("fixture", ["last_digit", "again", "replicates"])
def test_the_command_writes_the_twins_bytes_with_names(tmp_path, twin_texts, fixture, mode):
    named, tables, flags, (site, indiv) = twin_texts(fixture)
    assert len(site.splitlines()) > 1 and len(indiv.splitlines()) > 20
    out = str(tmp_path / "out")
    r = run(["eventalign_inference", "--out_dir", out, "--read_names", "--eventalign"] + as_list(named) + COMMON + flags + MODES[mode],
            env=dict(os.environ, M6A_EVENTALIGN_TIMES="1"), timeout=300)
    assert b"declined" not in r.stderr, r.stderr[-500:]
    if mode.startswith("gz"):
        assert not any(os.path.exists(os.path.join(out, f)) for f in CSVS)
        got = tuple(gzip.decompress(open(os.path.join(out, f + ".gz"), "rb").read()) for f in CSVS)
    else:
        got = tuple(open(os.path.join(out, f), "rb").read() for f in CSVS)
    want = RS.indiv(indiv, tables)
    assert got[0] == site and got[1] == want, (fixture, mode)
    if fixture == "replicates":                                # one name, two files: <uuid>_0 and <uuid>_1
        shared = NG.shared_in_pooled_sites(NG.replicates("split"))
        assert shared and all(RS.show(v) + b"_0," in got[1] and RS.show(v) + b"_1," in got[1] for v in shared)
    import json
    (line,) = [l for l in r.stdout.decode().splitlines() if l.startswith("M6A_TIMES ")]
    t = json.loads(line[len("M6A_TIMES "):])
    assert t["n_read_names"] == sum(map(len, tables)) and t["ms"]["intern"] > 0 and t["csv_writer"] == ("host" if mode == "host" else "device")


# ---- what is no name -------------------------------------------------------------------------------------------------------------------
def refused(path, text, **kw):
    with pytest.raises(_io.M6AIOError) as e:
        _io.prep_sites(path, n_threads=2, read_names=True, **kw)
    assert e.value.code == -4 and str(e.value).split(": ", 1)[1] == "%s: %s" % (path, text), (str(e.value), text)


def test_malformed_names_are_refused_at_the_lowest_offset(tmp_path):
    first = None
    for sp in sorted(NG.SPELLINGS):
        for place in NG.PLACES:
            data, at = NG.malformed(sp, place)
            p = tmp_path / ("%s_%s.txt" % (sp, place))
            p.write_bytes(data)
            text = "read name at byte %d: not a lowercase UUID" % at
            refused(str(p), text)
            if first is None:
                first = (str(p), text)
                refused(str(p), text, window_kb=4)
    for short_first in (True, False):
        data, text = NG.short_and_bad(short_first)
        p = tmp_path / ("both_%d.txt" % short_first)
        p.write_bytes(data)
        refused(str(p), text)
        refused(str(p), text, window_kb=4)
    # an indexed file under the flag is refused at its first body line; a named file without the flag is not this feature's business
    c = NG.case("last_digit")
    named, twin = c.write(tmp_path)
    at = c.twin.index(b"\n") + 1 + NG.fields(c.twin.split(b"\n")[1])[0]
    refused(twin, "read name at byte %d: not a lowercase UUID" % at)
    with _io.prep_sites(named, n_threads=2, read_names=True) as p:           # and the device is fine afterwards
        assert p.n_sites > 0
    out = str(tmp_path / "out")
    r = run(["eventalign_inference", "--out_dir", out, "--read_names", "--eventalign", first[0]] + COMMON, check=False, timeout=300)
    assert r.returncode != 0 and first[1].encode() in r.stderr
    assert not any(os.path.exists(os.path.join(out, f)) or os.path.exists(os.path.join(out, f + ".gz")) for f in CSVS)
