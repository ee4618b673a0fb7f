"""compute_norm_factors on the GPU: the kernels of m6a_norm_factors_build (m6anet_amd/csrc/m6a_norm.h, part 2) against the host route of
libm6a_io.so and against tests/norm_statement.py, bit for bit, on the golden directory and every generated family
(tests/norm_gen.py); what they decline, what comes back from the device, the budget, the errors and the command."""
import os
import subprocess
import sys

import numpy as np
import pytest

import json_statement as JS
import norm_gen as NG
import norm_statement as NS
from m6anet_amd import _io
from m6anet_amd.data_utils import load_norm_factors
from test_norm_factors import REPO, assert_route_is_statement, golden_dir, route, run_cli, same_bits

pytestmark = pytest.mark.gpu

NAMES = ["golden"] + list(NG.FAMILIES)


@pytest.fixture(scope="module")
def families(tmp_path_factory):
    """name -> (path, Train rows the statement calls declined, the statement's sums, the host route, the device route)"""
    root = tmp_path_factory.mktemp("norm_gpu")
    out = {}
    for name in NAMES:
        if name == "golden":
            path = golden_dir(root / "golden")
            with open(os.path.join(path, "data.json"), "rb") as f:
                blob = f.read()
            n_decl = sum(JS.walk(blob[a:b], tx, pos, n)[0] not in ("ok", "vocabulary") for tx, pos, a, b, n in NS.train_rows(path))
        else:
            d = NG.FAMILIES[name](str(root / name.replace(" ", "_")))
            path, n_decl = d.path, d.n_declined()
        out[name] = (path, n_decl, NS.sums(path), route(path), route(path, device=0))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_device_route_is_the_host_route_and_the_statement(families, name):
    path, n_decl, want, host, dev = families[name]
    assert_route_is_statement(dev, want, name)
    assert dev["kmers"] == host["kmers"] and dev["kmer7"] == host["kmer7"] and np.array_equal(dev["N"], host["N"])
    for f in ("S", "S2", "mean", "std"):
        assert same_bits(dev[f], host[f]), (name, f)
    # a condition, not a figure: the kernels take every site the statement calls regular
    st = dev["stats"]
    assert st["n_declined"] == n_decl == int((dev["status"] != 0).sum()), (name, st["n_declined"], n_decl)
    assert st["n_sites"] == len(dev["status"]) and st["n_kmers"] == len(want) and st["n_reads"] == sum(w[0] for w in want.values()) // 3


def test_declined_sites_give_their_regular_twins_bits(families):
    a, b = families["declined"][4], families["declined twin"][4]
    assert a["stats"]["n_declined"] == 5 and b["stats"]["n_declined"] == 0
    assert a["kmers"] == b["kmers"] and np.array_equal(a["N"], b["N"])
    for f in ("S", "S2", "mean", "std"):
        assert same_bits(a[f], b[f]), f
    n = families["nonfinite"][4]
    assert n["stats"]["n_declined"] == 3 and np.isnan(n["std"]).any() and not np.isnan(n["std"]).all()


def test_what_comes_back_does_not_grow_with_the_reads(families):
    a, b = families["scaled x1"][4]["stats"], families["scaled x10"][4]["stats"]
    assert b["n_reads"] == 10 * a["n_reads"] and a["n_sites"] == b["n_sites"] and a["n_kmers"] == b["n_kmers"]
    assert a["d2h_bytes"] == b["d2h_bytes"]
    for name in NAMES:
        st = families[name][4]["stats"]                          # a status byte and the 7-mer per site, 64 bytes per 5-mer, one count
        assert 0 < st["d2h_bytes"] <= 9 * st["n_sites"] + 64 * st["n_kmers"] + 8, (name, st)
        assert st["peak_bytes"] >= 72 * st["n_reads"]


CHILD = """
import sys
sys.path[:0] = [%r, %r]
from m6anet_amd import _io
from test_norm_factors import route
try:
    route(%r, device=0)
except _io.M6AIOError as e:
    print("CODE", e.code, str(e))
"""


def test_over_the_budget_is_enomem_naming_device_cpu(families):
    path = families["sizes"][0]
    assert os.path.getsize(os.path.join(path, "data.json")) > 2 << 20
    r = subprocess.run([sys.executable, "-c", CHILD % (REPO, os.path.join(REPO, "tests"), path)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, M6A_PREP_BUDGET_MB="2"))
    assert r.returncode == 0 and r.stdout.startswith("CODE -2 ") and "--device cpu" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_errors_are_the_host_routes_code_and_text(tmp_path):
    dirs = [NG.malformed(str(tmp_path / ("m%d" % k)), name) for k, name in enumerate(sorted(NG.MALFORMED_TEXT))]
    dirs.append(NG.out_of_range(str(tmp_path / "range")))
    for d in dirs:
        with pytest.raises(_io.M6AIOError) as h:
            route(d.path)
        with pytest.raises(_io.M6AIOError) as g:
            route(d.path, device=0)
        assert (g.value.code, str(g.value)) == (h.value.code, str(h.value)) and h.value.code == -4, (d.path, str(g.value), str(h.value))


def test_cli_on_the_gpu_writes_the_hosts_arrays(families, tmp_path):
    import json
    path = families["golden"][0]
    r = run_cli("--input_dir", path, "--out_dir", tmp_path / "gpu", env={"M6A_NORM_TIMES": "1"})            # --device gpu is the default
    assert r.returncode == 0, r.stderr[-2000:]
    assert run_cli("--input_dir", path, "--out_dir", tmp_path / "cpu", "--device", "cpu").returncode == 0
    for ext in (".npz", ".joblib"):
        a, b = (load_norm_factors(str(tmp_path / d / ("norm_dict_nanopolish" + ext))) for d in ("gpu", "cpu"))
        assert list(a) == list(b) and len(a) == 9
        assert all(same_bits(a[k][0], b[k][0]) and same_bits(a[k][1], b[k][1]) for k in a)
    t, = [json.loads(l[len("M6A_TIMES "):]) for l in r.stderr.splitlines() if l.startswith("M6A_TIMES ")]
    assert t["device"] == "gpu" and t["n_sites"] == 133 and t["n_declined"] == 0 and t["d2h_bytes"] > 0 and t["peak_device_bytes"] > 0
