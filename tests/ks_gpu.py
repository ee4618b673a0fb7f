"""What tests/test_gpu_ks.py and tests/test_gpu_signal_ks.py share: one call of m6a_site_ks or m6a_site_signal_ks through the engine's
*_ptrs method, with device or host pointers and a sentinel before and behind each of the four outputs."""
import numpy as np
import pytest

from m6anet_amd import _lib

FILL = 7
WHAT = ("d_pos", "d_neg", "med_a", "med_b")


def resident(cases):
    """the two sets of `cases` in device memory"""
    import torch
    va, oa, vb, ob, _ = cases.sets()
    return tuple(torch.from_numpy(x).cuda() for x in (va, oa, vb, ob))


def run(eng, cases, pointers, ia, ib, P, optional=True, sets=None, resident=None, deferred=False):
    """returns (d_pos, d_neg, med_a, med_b), each [P] or [P, 9], without the sentinels.  optional: med_a and med_b are asked for.
    deferred: the sync behind a device call must return M6A_EINVAL (the results are read after it)"""
    S, W = cases.n_sites(), cases.columns
    call = eng.site_ks_ptrs if W == 1 else eng.site_signal_ks_ptrs
    if pointers == "host":
        va, oa, vb, ob = sets or cases.sets()[:4]
        out = [np.full(W * P + 2, FILL, np.int64) for _ in range(2)] + [np.full(W * P + 2, float(FILL), np.float64) for _ in range(2)]
        keep = [np.ascontiguousarray(x, np.int64) if x is not None else None for x in (ia, ib)]
        ptr = lambda x, skip=0: None if x is None else x.ctypes.data + skip    # noqa: E731
        host = lambda x: x                                                       # noqa: E731
    else:
        import torch
        va, oa, vb, ob = sets or resident
        out = [torch.full((W * P + 2,), FILL, dtype=torch.int64, device="cuda:0") for _ in range(2)] + \
              [torch.full((W * P + 2,), float(FILL), dtype=torch.float64, device="cuda:0") for _ in range(2)]
        keep = [torch.from_numpy(np.ascontiguousarray(x, np.int64)).cuda() if x is not None else None for x in (ia, ib)]
        torch.cuda.synchronize()
        ptr = lambda x, skip=0: None if x is None else x.data_ptr() + skip      # noqa: E731
        host = lambda x: x.cpu().numpy()                                         # noqa: E731
    opt = [ptr(o, 8) if optional else None for o in out[2:]]
    call(ptr(va), ptr(oa), S, ptr(vb), ptr(ob), S, ptr(keep[0]), ptr(keep[1]), P, ptr(out[0], 8), ptr(out[1], 8), *opt)
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
    return [g[1:-1].reshape((P,) if W == 1 else (P, W)) for g in got]


def check_statement(eng, cases, res, pointers, name):
    ia, ib, P = cases.pairs(name)
    if name == "past the grid":                                  # four pairs per block: no grid of the launch covers the list in one pass
        import torch
        assert P > 4 * 64 * torch.cuda.get_device_properties(0).multi_processor_count
    want = cases.want(ia, ib)
    got = run(eng, cases, pointers, ia, ib, P, resident=res)
    for g, w, what in zip(got, want, WHAT):
        assert cases_same(g, w), (name, what, np.argwhere(g != w)[:5])
    d_pos, d_neg, med_a, med_b = run(eng, cases, pointers, ia, ib, P, optional=False, resident=res)     # the medians left out
    assert cases_same(d_pos, want[0]) and cases_same(d_neg, want[1]) and (med_a == FILL).all() and (med_b == FILL).all()


def cases_same(a, b):
    from ks_cases import same_bits
    return same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b))


def check_bad_host_arguments(eng, cases):
    """refused before anything runs, the outputs as they were; then a mixture of host and device pointers, and no pairs"""
    S, W = cases.n_sites(), cases.columns
    f = eng._L.m6a_site_ks if W == 1 else eng._L.m6a_site_signal_ks
    call = eng.site_ks_ptrs if W == 1 else eng.site_signal_ks_ptrs
    method = eng.site_ks if W == 1 else eng.site_signal_ks
    good = np.zeros(3, np.int64)
    for ia, ib, P in ((np.array([0, S, 1]), good, 3), (good, np.array([0, -1, 1]), 3), (None, None, S - 1), (good, None, 3)):
        with pytest.raises(_lib.M6AError) as e:
            run(eng, cases, "host", ia, ib, P)
        assert e.value.code == -1                                # M6A_EINVAL
    va, oa, vb, ob = cases.sets()[:4]
    for ia, ib in ((np.array([0, S, 1]), good), (good, np.array([0, -1, 1]))):       # ... and the outputs are as they were
        out = [np.full(3 * W, FILL, np.int64) for _ in range(2)] + [np.full(3 * W, float(FILL)) for _ in range(2)]
        rc = f(eng._h, va.ctypes.data, oa.ctypes.data, S, vb.ctypes.data, ob.ctypes.data, S, np.ascontiguousarray(ia, np.int64).ctypes.data,
               np.ascontiguousarray(ib, np.int64).ctypes.data, 3, *[o.ctypes.data for o in out])
        assert rc == -1 and all((o == FILL).all() for o in out)
    for bad in (np.array([1, 2, 3], np.int64), np.array([0, 2, 1], np.int64)):       # offsets that do not start at 0, that decrease
        with pytest.raises(_lib.M6AError) as e:
            method(va, bad, vb, ob[:3].copy())
        assert e.value.code == -1
    d = np.full(W * S, FILL, np.int64)
    for d_pos, d_neg in ((None, d.ctypes.data), (d.ctypes.data, None)):              # d_pos and d_neg are required
        with pytest.raises(_lib.M6AError) as e:
            call(va.ctypes.data, oa.ctypes.data, S, vb.ctypes.data, ob.ctypes.data, S, None, None, S, d_pos, d_neg, None, None)
        assert e.value.code == -1
    import torch
    dev_va = torch.from_numpy(va).cuda()
    with pytest.raises(_lib.M6AError) as e:                      # a mixture of host and device pointers
        call(dev_va.data_ptr(), oa.ctypes.data, S, vb.ctypes.data, ob.ctypes.data, S, None, None, S, d.ctypes.data, d.ctypes.data, None, None)
    assert e.value.code == -1 and (d == FILL).all()
    assert f(eng._h, None, None, 0, None, None, 0, None, None, 0, None, None, None, None) == 0     # no pairs: M6A_OK


def check_bad_device_index(eng, cases, res):
    """contained -- the undefined values for the bad pairs alone -- and reported by the next sync; the context goes on afterwards"""
    S = cases.n_sites()
    ia, ib = (x.copy() for x in cases.pair_lists()["65 drawn"])
    want = [w.copy() for w in cases.want(ia, ib)]
    for k, (a, b) in ((3, (S, ib[3])), (40, (ia[40], -1)), (64, (1 << 40, ib[64]))):
        ia[k], ib[k] = a, b
        want[0][k] = want[1][k] = -1                             # every column of the pair
        want[2][k] = want[3][k] = np.nan
    got = run(eng, cases, "device", ia, ib, 65, resident=res, deferred=True)
    assert all(cases_same(g, w) for g, w in zip(got, want))
    va, oa, vb, ob = res
    bad_off = oa.clone()
    bad_off[5] = oa[6] + 1                                       # site 4 now ends inside site 6; site 5 runs backwards
    got = run(eng, cases, "device", None, None, S, sets=(va, bad_off, vb, ob), deferred=True)
    keep = ~np.isin(np.arange(S), (4, 5))                        # site 4 is another bag now: defined, not the statement's
    for g, w in zip(got[:2], cases.want()[:2]):
        assert (g[5] == -1).all() and (g[4] >= 0).all() and cases_same(g[keep], w[keep])
    for g, w in zip(got[2:], cases.want()[2:]):
        assert np.isnan(g[5]).all() and cases_same(g[keep], w[keep])
    ia, ib = cases.pair_lists()["1 drawn"]
    assert all(cases_same(g, w) for g, w in zip(run(eng, cases, "device", ia, ib, 1, resident=res), cases.want(ia, ib)))   # the context goes on
