"""m6a_site_ks on the GPU (include/m6a.h): site_ks_kernel gives the two integers and the medians' bits that tests/ks_statement.py states,
with device pointers and with host pointers, on every shape of tests/ks_cases.py -- those of tests/ranksum_cases.py (bag sizes around the
wavefront's chunk of 64 crossed, lopsided pairs, pairs around the LDS tile of 256 floats, a 3000 x 2500 pair, empty bags, ties, signed
zeros, infinities, NaN) and the ones new here (a bimodal bag against a unimodal one of the same median, odd and even sizes, middles of
-0.0 and 0.0, middles of -inf and +inf) -- for every list of ks_cases.LISTS: sites repeated, backwards, 0, 1, 65 and 4097 pairs, the
identity, more pairs than the largest grid covers.  Sentinels sit around all four outputs; the medians may be left out.  A bad index is
refused on the host, and contained and reported on the device, after which the context goes on."""
import numpy as np
import pytest

import ks_cases as KC
import ks_gpu
from m6anet_amd.engine import M6ANetEngine

pytestmark = pytest.mark.gpu
CASES = KC.scalar


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
        pa, oa, pb, ob = CASES.sets()[:4]
        got = eng.site_ks(pa, oa, pb, ob, ia, ib)
        ident = eng.site_ks(pa, oa, pb, ob)
    else:
        import torch
        got = eng.site_ks(*resident, torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda())
        ident = eng.site_ks(*resident)
        eng.sync()
        got, ident = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in ident]
    assert all(g.shape == (65,) for g in got)
    assert all(KC.same_bits(g, w) for g, w in zip(got, CASES.want(ia, ib)))
    assert all(KC.same_bits(g, w) for g, w in zip(ident, CASES.want()))
    with pytest.raises(ValueError):
        eng.site_ks(*CASES.sets()[:4], ia, None)


def test_the_bimodal_pair_on_the_device(eng, resident):
    """the pair this call exists for, through both kernels: the rank-sum's |z| stays below 1 where ks_d is 0.5"""
    import torch
    from m6anet_amd import ranksum
    k = torch.tensor([CASES.site_of("bimodal against unimodal")], device="cuda:0")
    z = eng.site_ranksum(*resident, k, k)[3]
    d_pos, d_neg, med_a, med_b = eng.site_ks(*resident, k, k)
    eng.sync()
    assert abs(float(z[0])) < 1 and float(med_a[0]) == float(med_b[0]) == 0.5
    assert ranksum.ks_d(d_pos.cpu().numpy(), d_neg.cpu().numpy(), [60], [61])[0] == 0.5 > 0.3


def test_bad_arguments_on_host_arrays_are_refused_before_anything_runs(eng):
    ks_gpu.check_bad_host_arguments(eng, CASES)


def test_bad_index_in_device_arrays_is_contained_and_reported(eng, resident):
    ks_gpu.check_bad_device_index(eng, CASES, resident)
    assert np.isfinite(CASES.want()[2][:len(KC.RC.SIZES)]).all()
