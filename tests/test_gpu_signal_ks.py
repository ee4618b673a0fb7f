"""m6a_site_signal_ks on the GPU (include/m6a.h): site_signal_ks_kernel gives the integers and the medians' bits that tests/ks_statement.py
states per column, with device pointers and with host pointers, on every shape of tests/ks_cases.py -- those of
tests/signal_ranksum_cases.py (bag sizes around the wavefront's chunk of 64 and around the LDS tile of 256 rows crossed, a 3000 x 2500
pair, a value family per column, NaN in one column of one side and in all, signed zeros, infinities, empty bags) and the ones new here,
each in a column of its own -- for every list of ks_cases.LISTS.  Sentinels sit around all four outputs; the medians may be left out.  A
bad index is refused on the host, and contained and reported on the device, after which the context goes on.  Column 0 is what
m6a_site_ks gives on a contiguous copy of column 0."""
import numpy as np
import pytest

import ks_cases as KC
import ks_gpu
from m6anet_amd.engine import M6ANetEngine

pytestmark = pytest.mark.gpu
CASES = KC.signal


@pytest.fixture(scope="module")
def eng(weights):
    e = M6ANetEngine(weights=weights["hct116"], device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def resident():
    return ks_gpu.resident(CASES)


@pytest.mark.parametrize("pointers", ["device", "host"])
@pytest.mark.parametrize("name", KC.LISTS)
def test_kernel_gives_the_statement(eng, resident, pointers, name):
    ks_gpu.check_statement(eng, CASES, resident, pointers, name)


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_engine_method_on_arrays_and_tensors(eng, resident, pointers):
    ia, ib = CASES.pair_lists()["65 drawn"]
    if pointers == "host":
        Xa, oa, Xb, ob = CASES.sets()[:4]
        got = eng.site_signal_ks(Xa, oa, Xb, ob, ia, ib)
        ident = eng.site_signal_ks(Xa, oa, Xb, ob)
    else:
        import torch
        got = eng.site_signal_ks(*resident, torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda())
        ident = eng.site_signal_ks(*resident)
        eng.sync()
        got, ident = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in ident]
    assert all(g.shape == (65, 9) for g in got)
    assert all(KC.same_bits(g, w) for g, w in zip(got, CASES.want(ia, ib)))
    assert all(KC.same_bits(g, w) for g, w in zip(ident, CASES.want()))
    with pytest.raises(ValueError):
        eng.site_signal_ks(*CASES.sets()[:4], ia, None)


def test_column_0_is_site_ks_on_a_copy_of_column_0(eng, resident):
    """the two kernels tied together, on the device: m6a_site_ks on contiguous copies of column 0 of both sets"""
    import torch
    Xa, oa, Xb, ob = resident
    ia, ib = (torch.from_numpy(x).cuda() for x in CASES.pair_lists()["crossed and special"])
    nine = eng.site_signal_ks(Xa, oa, Xb, ob, ia, ib)
    one = eng.site_ks(Xa[:, 0].contiguous(), oa, Xb[:, 0].contiguous(), ob, ia, ib)
    eng.sync()
    for g, w in zip(nine, one):
        assert KC.same_bits(np.ascontiguousarray(g.cpu().numpy()[:, 0]), w.cpu().numpy())


def test_bad_arguments_on_host_arrays_are_refused_before_anything_runs(eng):
    ks_gpu.check_bad_host_arguments(eng, CASES)


def test_bad_index_in_device_arrays_is_contained_and_reported(eng, resident):
    ks_gpu.check_bad_device_index(eng, CASES, resident)
