"""m6a_site_ranksum on the GPU (include/m6a.h): site_ranksum_kernel gives the integers and the bits of z that tests/ranksum_statement.py
states, with device pointers and with host pointers, on every shape of tests/ranksum_cases.py -- bag sizes around the wavefront's
chunk of 64 crossed, lopsided pairs, pairs around the LDS tile of 256 floats (ranksum_cases.TILE = M6A_PAIR_TILE), a 3000 x 2500
pair, empty bags, ties, signed zeros, infinities, NaN -- for pair lists that repeat sites, run backwards and hold 0, 1, 65 and 4097
pairs, with the index arrays and the optional outputs left out, and with sentinels around all four outputs.  A bad index is refused on
the host and contained on the device."""
import numpy as np
import pytest

import ranksum_cases as RC
from m6anet_amd import _lib
from m6anet_amd.engine import M6ANetEngine

pytestmark = pytest.mark.gpu
FILL = 7


@pytest.fixture(scope="module")
def eng(weights):
    e = M6ANetEngine(weights=weights["hct116"], device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def resident():
    """the two sets of ranksum_cases.sets() in device memory"""
    import torch
    pa, oa, pb, ob, _ = RC.sets()
    return tuple(torch.from_numpy(x).cuda() for x in (pa, oa, pb, ob))


def run(eng, pointers, ia, ib, P, optional=True, sets=None, resident=None, deferred=False):
    """m6a_site_ranksum through site_ranksum_ptrs with a sentinel before and behind each output; returns (gt, eq, tie, z) without them.
    deferred: the sync behind a device call must return M6A_EINVAL (the results are read after it)"""
    S = RC.n_sites()
    if pointers == "host":
        pa, oa, pb, ob = sets or RC.sets()[:4]
        out = [np.full(P + 2, FILL, np.int64) for _ in range(3)] + [np.full(P + 2, float(FILL), np.float64)]
        keep = [np.ascontiguousarray(x, np.int64) if x is not None else None for x in (ia, ib)]
        ptr = lambda x, skip=0: None if x is None else x.ctypes.data + skip    # noqa: E731
        host = lambda x: x                                                       # noqa: E731
    else:
        import torch
        pa, oa, pb, ob = sets or resident
        out = [torch.full((P + 2,), FILL, dtype=torch.int64, device="cuda:0") for _ in range(3)] + \
              [torch.full((P + 2,), float(FILL), dtype=torch.float64, device="cuda:0")]
        keep = [torch.from_numpy(np.ascontiguousarray(x, np.int64)).cuda() if x is not None else None for x in (ia, ib)]
        torch.cuda.synchronize()
        ptr = lambda x, skip=0: None if x is None else x.data_ptr() + skip      # noqa: E731
        host = lambda x: x.cpu().numpy()                                         # noqa: E731
    opt = [ptr(o, 8) if optional else None for o in out[:3]]
    eng.site_ranksum_ptrs(ptr(pa), ptr(oa), S, ptr(pb), ptr(ob), S, ptr(keep[0]), ptr(keep[1]), P, *opt, ptr(out[3], 8))
    if pointers == "device" and deferred:
        with pytest.raises(_lib.M6AError) as e:
            eng.sync()
        assert e.value.code == -1                                # M6A_EINVAL
        eng.sync()                                               # reported once
    elif pointers == "device":
        eng.sync()
    got = [host(o) for o in out]
    for g in got:
        assert g[0] == FILL and g[-1] == FILL
    return [g[1:-1] for g in got]


@pytest.mark.parametrize("pointers", ["device", "host"])
@pytest.mark.parametrize("name", ["crossed and special", "backwards", "0 drawn", "1 drawn", "65 drawn", "4097 drawn", "identity"])
def test_kernel_gives_the_statement(eng, resident, pointers, name):
    ia, ib = (None, None) if name == "identity" else RC.pair_lists()[name]
    P = RC.n_sites() if ia is None else ia.size
    want = RC.want(ia, ib)
    got = run(eng, pointers, ia, ib, P, resident=resident)
    for g, w, what in zip(got, want, ("gt", "eq", "tie", "z")):
        assert RC.same_bits(g, w), (name, what, np.flatnonzero(g != w)[:5])
    gt, eq, tie, z = run(eng, pointers, ia, ib, P, optional=False, resident=resident)      # gt, eq and tie left out: z alone is written
    assert RC.same_bits(z, want[3]) and (gt == FILL).all() and (eq == FILL).all() and (tie == FILL).all()


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_engine_method_on_arrays_and_tensors(eng, resident, pointers):
    ia, ib = RC.pair_lists()["65 drawn"]
    if pointers == "host":
        pa, oa, pb, ob = RC.sets()[:4]
        got = eng.site_ranksum(pa, oa, pb, ob, ia, ib)
        ident = eng.site_ranksum(pa, oa, pb, ob)
    else:
        import torch
        got = eng.site_ranksum(*resident, torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda())
        ident = eng.site_ranksum(*resident)
        eng.sync()
        got, ident = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in ident]
    assert all(RC.same_bits(g, w) for g, w in zip(got, RC.want(ia, ib)))
    assert all(RC.same_bits(g, w) for g, w in zip(ident, RC.want()))
    with pytest.raises(ValueError):
        eng.site_ranksum(*RC.sets()[:4], ia, None)


def test_bad_arguments_on_host_arrays_are_refused_before_anything_runs(eng):
    S = RC.n_sites()
    good = np.zeros(3, np.int64)
    for ia, ib, P in ((np.array([0, S, 1]), good, 3), (good, np.array([0, -1, 1]), 3), (None, None, S - 1), (good, None, 3)):
        with pytest.raises(_lib.M6AError) as e:
            run(eng, "host", ia, ib, P)
        assert e.value.code == -1                                # M6A_EINVAL
    pa, oa, pb, ob = RC.sets()[:4]
    for ia, ib in ((np.array([0, S, 1]), good), (good, np.array([0, -1, 1]))):       # ... and the outputs are as they were
        out = [np.full(3, FILL, np.int64) for _ in range(3)] + [np.full(3, float(FILL))]
        rc = eng._L.m6a_site_ranksum(eng._h, pa.ctypes.data, oa.ctypes.data, S, pb.ctypes.data, ob.ctypes.data, S,
                                     np.ascontiguousarray(ia, np.int64).ctypes.data, np.ascontiguousarray(ib, np.int64).ctypes.data, 3,
                                     *[o.ctypes.data for o in out])
        assert rc == -1 and all((o == FILL).all() for o in out)
    for bad in (np.array([1, 2, 3], np.int64), np.array([0, 2, 1], np.int64)):       # offsets that do not start at 0, that decrease
        with pytest.raises(_lib.M6AError) as e:
            eng.site_ranksum(pa, bad, pb, ob[:3].copy())
        assert e.value.code == -1
    import torch
    dev_pa, z = torch.from_numpy(pa).cuda(), np.zeros(S)
    with pytest.raises(_lib.M6AError) as e:                      # a mixture of host and device pointers
        eng.site_ranksum_ptrs(dev_pa.data_ptr(), oa.ctypes.data, S, pb.ctypes.data, ob.ctypes.data, S, None, None, S, None, None, None,
                              z.ctypes.data)
    assert e.value.code == -1
    assert eng._L.m6a_site_ranksum(eng._h, None, None, 0, None, None, 0, None, None, 0, None, None, None, None) == 0     # no pairs: M6A_OK


def test_bad_index_in_device_arrays_is_contained_and_reported(eng, resident):
    S = RC.n_sites()
    ia, ib = (x.copy() for x in RC.pair_lists()["65 drawn"])
    want = [w.copy() for w in RC.want(ia, ib)]
    for k, (a, b) in ((3, (S, ib[3])), (40, (ia[40], -1)), (64, (1 << 40, ib[64]))):
        ia[k], ib[k] = a, b
        want[0][k] = want[1][k] = want[2][k] = -1
        want[3][k] = np.nan
    got = run(eng, "device", ia, ib, 65, resident=resident, deferred=True)
    assert all(RC.same_bits(g, w) for g, w in zip(got, want))                # the undefined pair's values for those three pairs alone
    pa, oa, pb, ob = resident
    bad_off = oa.clone()
    bad_off[5] = oa[6] + 1                                                   # site 4 now ends inside site 6; site 5 runs backwards
    got = run(eng, "device", None, None, S, sets=(pa, bad_off, pb, ob), deferred=True)
    keep = ~np.isin(np.arange(S), (4, 5))                                    # site 4 is another bag now: defined, not the statement's
    for g, w in zip(got[:3], RC.want()[:3]):
        assert g[5] == -1 and g[4] >= 0 and RC.same_bits(g[keep], w[keep])
    assert np.isnan(got[3][5]) and not np.isnan(got[3][4]) and RC.same_bits(got[3][keep], RC.want()[3][keep])
    ia, ib = RC.pair_lists()["1 drawn"]
    assert all(RC.same_bits(g, w) for g, w in zip(run(eng, "device", ia, ib, 1, resident=resident), RC.want(ia, ib)))   # the context goes on
