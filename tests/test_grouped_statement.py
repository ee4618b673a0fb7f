"""`eventalign_inference --grouped` on the host side: the grouped rule (tests/grouped_statement.py) on the generated families and on
tests/grouped_gen.py's files, the prefix property of m6a_flush_groups that lets a batch start on a boundary of a job whose length is
not known yet, and the four combinations the flag refuses as argument errors before anything is opened."""
import numpy as np
import pytest

import eventalign_gen as G
import grouped_gen as GG
import grouped_statement as GS
from m6anet_amd import engine

GROUPED = ["plain", "radix_4095", "radix_4096", "radix_4097", "radix_8192", "radix_ties", "numbers_ok", "atoll", "combine", "windows_2",
           "windows_3", "declined"]
NOT_GROUPED = ["split_runs", "split_rows", "newlines_0", "newlines_1", "newlines_2", "filters_20", "filters_25"]


def test_the_families_split_as_expected():
    """so that the GPU tests are known to see both kinds"""
    for family in GROUPED:
        assert GS.offender(G.case(family, 1).data) is None, family
    for family in NOT_GROUPED:
        data = G.case(family, 1).data
        name, start = GS.offender(data)
        assert data[start:start + len(name) + 1] == name + b"\t" and (start == 0 or data[start - 1:start] == b"\n"), family
        assert data.count(b"\n" + name + b"\t", 0, start) >= 1, family        # the name was there before


def test_the_offender_is_the_first_run_that_comes_back():
    f = G.File(np.random.default_rng(1))
    a, b, c = (f.text(contig, 5, "GGACT", 1) for contig in ("A", "B", "C"))
    h = G.HEADER
    assert GS.grouped(h) and GS.grouped(h + a + a + b + c)
    assert GS.offender(h + a + b + a + c + b) == (b"A", len(h + a + b))
    assert GS.offender(h + a + b + b"no tab here\n" + c + b) == (b"B", len(h + a + b) + len(b"no tab here\n") + len(c))
    assert GS.grouped(h + a + b"\n" + a + b)                                  # a line without a tab ends no stretch
    name, start = GS.offender(h + a + b + a)
    assert GS.error_text("ev.txt", name, start) == ("ev.txt: transcript A appears again at byte %d after other transcripts: the input is not "
                                                    "grouped by transcript (run without --grouped)" % start)


def test_the_generators_files():
    for name in GG.GROUPED_FILES:
        assert GS.grouped(GG.file(name)), name
    many = GG.file("many")
    assert 32 * 80_000 < len(many) < 32 * 140_000
    assert GS.offender(GG.file("moved")) == GG.moved_offender()
    name, at = GG.moved_offender()
    assert name.startswith(b"GRP%03d." % GG.MOVED_TX) and sorted(GG.file("moved")) == sorted(many)


@pytest.mark.parametrize("save_per_batch", [1, 2, 3, 4])
def test_flush_boundaries_of_a_longer_job_extend_those_of_a_shorter_one(save_per_batch):
    """m6a_flush_groups: the boundaries depend on the batch index alone, so a longer job's boundaries are a shorter job's, apart from
    the shorter job's final group, and then more; with 16 / 2 they fall at 16, 48, 80, ..."""
    for batch_size in (1, 3, 16):
        longest = [int(x) for x in engine.flush_groups(40 * batch_size + 1, batch_size, save_per_batch)]
        assert longest[1:-1] == GS.flush_boundaries(40 * batch_size + 1, batch_size, save_per_batch)
        for n in range(0, 12 * batch_size + 2):
            g = [int(x) for x in engine.flush_groups(n, batch_size, save_per_batch)]
            assert g[0] == 0 and g[-1] == n
            inner = g[1:-1] if n else []
            assert inner == [x for x in longest[1:-1] if x < n], (n, batch_size, save_per_batch)
            # a job that ends on a boundary has written all its sites, so the cut of --drop_unflushed_tail in a later batch, the job's
            # written sites less the sites of the batches before, is never negative
            if n in longest[1:-1]:
                assert engine.reference_written_sites(n, batch_size, save_per_batch) == n, n
            assert engine.reference_written_sites(n, batch_size, save_per_batch) >= max([x for x in longest[1:-1] if x <= n], default=0), n
    if save_per_batch == 2:
        assert [int(x) for x in engine.flush_groups(101, 16, 2)][1:-1] == [16, 48, 80]


def test_the_four_refusals_are_exit_status_2_before_anything_is_opened(tmp_path, capsys):
    from m6anet_amd.__main__ import main
    ev = tmp_path / "missing.txt"                                              # never opened: it does not exist
    cases = [
        (["--eventalign", str(ev), str(ev)], "--grouped takes one --eventalign file"),
        (["--eventalign", str(ev), "--read_names"], "--grouped with --read_names"),
        (["--eventalign", str(ev), "--compress"], "--grouped with --compress"),
        (["--eventalign", str(ev), "--read_representation"], "--grouped with --read_representation"),
    ]
    for k, (argv, word) in enumerate(cases):
        out = tmp_path / ("out%d" % k)
        with pytest.raises(SystemExit) as e:
            main(["eventalign_inference", "--grouped", "--out_dir", str(out)] + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and word in err, (argv, e.value.code, err[-500:])
        assert not out.exists(), argv
    sentences = {word for _, word in cases}
    assert len(sentences) == 4
