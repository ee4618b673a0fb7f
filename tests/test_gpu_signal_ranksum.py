"""m6a_site_signal_ranksum on the GPU (include/m6a.h): site_signal_ranksum_kernel gives the integers and the bits of z that
tests/signal_ranksum_statement.py states, with device pointers and with host pointers, on every shape of tests/signal_ranksum_cases.py
-- bag sizes around the wavefront's chunk of 64 and around the LDS tile of 256 rows crossed, a 3000 x 2500 pair, a value family per
column, NaN in one column of one side and in all, signed zeros, infinities, empty bags -- for pair lists that repeat sites, run
backwards, hold 0, 1, 65 and 4097 pairs and outrun the largest grid, with the index arrays and the optional outputs left out, and with
sentinels around all four outputs.  A bad index is refused on the host and contained on the device.  Column 0 is what
m6a_site_ranksum gives on a contiguous copy of column 0."""
import numpy as np
import pytest

import signal_ranksum_cases as SC
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
    """the two sets of signal_ranksum_cases.sets() in device memory"""
    import torch
    Xa, oa, Xb, ob, _ = SC.sets()
    return tuple(torch.from_numpy(x).cuda() for x in (Xa, oa, Xb, ob))


def run(eng, pointers, ia, ib, P, optional=True, sets=None, resident=None, deferred=False):
    """m6a_site_signal_ranksum through site_signal_ranksum_ptrs with a sentinel before and behind each output; returns (gt, eq, tie, z),
    each [P, 9], without them.  deferred: the sync behind a device call must return M6A_EINVAL (the results are read after it)"""
    S = SC.n_sites()
    if pointers == "host":
        Xa, oa, Xb, ob = sets or SC.sets()[:4]
        out = [np.full(9 * P + 2, FILL, np.int64) for _ in range(3)] + [np.full(9 * P + 2, float(FILL), np.float64)]
        keep = [np.ascontiguousarray(x, np.int64) if x is not None else None for x in (ia, ib)]
        ptr = lambda x, skip=0: None if x is None else x.ctypes.data + skip    # noqa: E731
        host = lambda x: x                                                       # noqa: E731
    else:
        import torch
        Xa, oa, Xb, ob = sets or resident
        out = [torch.full((9 * P + 2,), FILL, dtype=torch.int64, device="cuda:0") for _ in range(3)] + \
              [torch.full((9 * P + 2,), float(FILL), dtype=torch.float64, device="cuda:0")]
        keep = [torch.from_numpy(np.ascontiguousarray(x, np.int64)).cuda() if x is not None else None for x in (ia, ib)]
        torch.cuda.synchronize()
        ptr = lambda x, skip=0: None if x is None else x.data_ptr() + skip      # noqa: E731
        host = lambda x: x.cpu().numpy()                                         # noqa: E731
    opt = [ptr(o, 8) if optional else None for o in out[:3]]
    eng.site_signal_ranksum_ptrs(ptr(Xa), ptr(oa), S, ptr(Xb), ptr(ob), S, ptr(keep[0]), ptr(keep[1]), P, *opt, ptr(out[3], 8))
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
    return [g[1:-1].reshape(P, 9) for g in got]


@pytest.mark.parametrize("pointers", ["device", "host"])
@pytest.mark.parametrize("name", SC.LISTS)
def test_kernel_gives_the_statement(eng, resident, pointers, name):
    ia, ib = (None, None) if name == "identity" else SC.pair_lists()[name]
    P = SC.n_sites() if ia is None else ia.size
    if name == "past the grid":                                  # four pairs per block: no grid of the launch covers the list in one pass
        import torch
        assert P > 4 * 64 * torch.cuda.get_device_properties(0).multi_processor_count
    want = SC.want(ia, ib)
    got = run(eng, pointers, ia, ib, P, resident=resident)
    for g, w, what in zip(got, want, ("gt", "eq", "tie", "z")):
        assert SC.same_bits(g, w), (name, what, np.argwhere(g != w)[:5])
    gt, eq, tie, z = run(eng, pointers, ia, ib, P, optional=False, resident=resident)      # gt, eq and tie left out: z alone is written
    assert SC.same_bits(z, want[3]) and (gt == FILL).all() and (eq == FILL).all() and (tie == FILL).all()


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_engine_method_on_arrays_and_tensors(eng, resident, pointers):
    ia, ib = SC.pair_lists()["65 drawn"]
    if pointers == "host":
        Xa, oa, Xb, ob = SC.sets()[:4]
        got = eng.site_signal_ranksum(Xa, oa, Xb, ob, ia, ib)
        ident = eng.site_signal_ranksum(Xa, oa, Xb, ob)
    else:
        import torch
        got = eng.site_signal_ranksum(*resident, torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda())
        ident = eng.site_signal_ranksum(*resident)
        eng.sync()
        got, ident = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in ident]
    assert all(g.shape == (65, 9) for g in got)
    assert all(SC.same_bits(g, w) for g, w in zip(got, SC.want(ia, ib)))
    assert all(SC.same_bits(g, w) for g, w in zip(ident, SC.want()))
    with pytest.raises(ValueError):
        eng.site_signal_ranksum(*SC.sets()[:4], ia, None)


def test_column_0_is_site_ranksum_on_a_copy_of_column_0(eng, resident):
    """the two kernels tied together, on the device: m6a_site_ranksum on contiguous copies of column 0 of both sets"""
    import torch
    Xa, oa, Xb, ob = resident
    ia, ib = (torch.from_numpy(x).cuda() for x in SC.pair_lists()["crossed and special"])
    nine = eng.site_signal_ranksum(Xa, oa, Xb, ob, ia, ib)
    one = eng.site_ranksum(Xa[:, 0].contiguous(), oa, Xb[:, 0].contiguous(), ob, ia, ib)
    eng.sync()
    for g, w in zip(nine, one):
        assert SC.same_bits(np.ascontiguousarray(g.cpu().numpy()[:, 0]), w.cpu().numpy())


def test_bad_arguments_on_host_arrays_are_refused_before_anything_runs(eng):
    S = SC.n_sites()
    good = np.zeros(3, np.int64)
    for ia, ib, P in ((np.array([0, S, 1]), good, 3), (good, np.array([0, -1, 1]), 3), (None, None, S - 1), (good, None, 3)):
        with pytest.raises(_lib.M6AError) as e:
            run(eng, "host", ia, ib, P)
        assert e.value.code == -1                                # M6A_EINVAL
    Xa, oa, Xb, ob = SC.sets()[:4]
    for ia, ib in ((np.array([0, S, 1]), good), (good, np.array([0, -1, 1]))):       # ... and the outputs are as they were
        out = [np.full(27, FILL, np.int64) for _ in range(3)] + [np.full(27, float(FILL))]
        rc = eng._L.m6a_site_signal_ranksum(eng._h, Xa.ctypes.data, oa.ctypes.data, S, Xb.ctypes.data, ob.ctypes.data, S,
                                            np.ascontiguousarray(ia, np.int64).ctypes.data, np.ascontiguousarray(ib, np.int64).ctypes.data, 3,
                                            *[o.ctypes.data for o in out])
        assert rc == -1 and all((o == FILL).all() for o in out)
    for bad in (np.array([1, 2, 3], np.int64), np.array([0, 2, 1], np.int64)):       # offsets that do not start at 0, that decrease
        with pytest.raises(_lib.M6AError) as e:
            eng.site_signal_ranksum(Xa, bad, Xb, ob[:3].copy())
        assert e.value.code == -1
    z = np.full(9 * S, float(FILL))
    with pytest.raises(_lib.M6AError) as e:                      # z is required
        eng.site_signal_ranksum_ptrs(Xa.ctypes.data, oa.ctypes.data, S, Xb.ctypes.data, ob.ctypes.data, S, None, None, S, None, None, None, None)
    assert e.value.code == -1
    import torch
    dev_Xa = torch.from_numpy(Xa).cuda()
    with pytest.raises(_lib.M6AError) as e:                      # a mixture of host and device pointers
        eng.site_signal_ranksum_ptrs(dev_Xa.data_ptr(), oa.ctypes.data, S, Xb.ctypes.data, ob.ctypes.data, S, None, None, S, None, None, None,
                                     z.ctypes.data)
    assert e.value.code == -1 and (z == FILL).all()
    assert eng._L.m6a_site_signal_ranksum(eng._h, None, None, 0, None, None, 0, None, None, 0, None, None, None, None) == 0     # no pairs: M6A_OK


def test_bad_index_in_device_arrays_is_contained_and_reported(eng, resident):
    S = SC.n_sites()
    ia, ib = (x.copy() for x in SC.pair_lists()["65 drawn"])
    want = [w.copy() for w in SC.want(ia, ib)]
    for k, (a, b) in ((3, (S, ib[3])), (40, (ia[40], -1)), (64, (1 << 40, ib[64]))):
        ia[k], ib[k] = a, b
        want[0][k] = want[1][k] = want[2][k] = -1                # all nine columns of the pair
        want[3][k] = np.nan
    got = run(eng, "device", ia, ib, 65, resident=resident, deferred=True)
    assert all(SC.same_bits(g, w) for g, w in zip(got, want))                # the undefined values for those three pairs alone
    Xa, oa, Xb, ob = resident
    bad_off = oa.clone()
    bad_off[5] = oa[6] + 1                                                   # site 4 now ends inside site 6; site 5 runs backwards
    got = run(eng, "device", None, None, S, sets=(Xa, bad_off, Xb, ob), deferred=True)
    keep = ~np.isin(np.arange(S), (4, 5))                                    # site 4 is another bag now: defined, not the statement's
    for g, w in zip(got[:3], SC.want()[:3]):
        assert (g[5] == -1).all() and (g[4] >= 0).all() and SC.same_bits(g[keep], w[keep])
    assert np.isnan(got[3][5]).all() and not np.isnan(got[3][4]).any() and SC.same_bits(got[3][keep], SC.want()[3][keep])
    ia, ib = SC.pair_lists()["1 drawn"]
    assert all(SC.same_bits(g, w) for g, w in zip(run(eng, "device", ia, ib, 1, resident=resident), SC.want(ia, ib)))   # the context goes on
