"""The encoder's A/B and timeline tools build their variants as text edits of a copy of m6a_kernels.hip (tools/variant_build.py): the
shipped source carries no experiment switch, and every edit must still find its anchors in it.  Pure string work, no compiler."""
import glob
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import encoder_ab  # noqa: E402
import encoder_timeline  # noqa: E402
import variant_build  # noqa: E402

VARIANTS = [(m, n) for m in (encoder_ab, encoder_timeline) for n in m.VARIANTS]


def test_no_ab_macro_in_shipped_source():
    files = glob.glob(os.path.join(REPO, "m6anet_amd", "csrc", "*")) + glob.glob(os.path.join(REPO, "include", "*"))
    assert len(files) > 10
    hits = [os.path.relpath(f, REPO) for f in files if os.path.isfile(f) and b"M6A_AB_" in open(f, "rb").read()]
    assert hits == []


def test_variant_lists():
    assert "base" in encoder_ab.VARIANTS and "no_epilogue" in encoder_ab.VARIANTS
    assert sum(n.startswith("links_") for n in encoder_ab.VARIANTS) == 9
    assert sorted(encoder_timeline.VARIANTS) == ["stamps", "stamps_body3_epi0", "stamps_noprio"]


@pytest.mark.parametrize("module,name", VARIANTS, ids=["%s-%s" % (m.__name__, n) for m, n in VARIANTS])
def test_variant_applies_to_tracked_source(module, name):
    src = variant_build.source("m6a_kernels.hip")
    out = module.VARIANTS[name](src)          # asserts its anchors
    assert (out == src) == (name == "base")
