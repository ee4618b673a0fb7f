"""m6a_ks_exact on the GPU (include/m6a.h): ks_exact_kernel gives the host core's bits (m6a_io_ks_exact, which tests/test_ks_exact_core.py
holds to tests/ks_exact_statement.py on the same items), compared as uint64, with device pointers and with host pointers and a sentinel
before and behind p.  The items are tests/ks_exact_cases.py's: sizes around the stripe of 64 rows crossed on both axes with h from the
undefined -1 over 0, the narrowest band and the middle to the band that covers the grid; both caps at the cap and one past it, on either
axis; a subnormal and a zero result; every item with its bags swapped; and one launch of more items than four per block of the largest
grid, in which the four wavefronts of a block get very different amounts of work.  No items, a null pointer and a mixture of host and
device pointers are M6A_OK, M6A_EINVAL and M6A_EINVAL with p as it was."""
import numpy as np
import pytest

import ks_exact_cases as KE
from m6anet_amd import _lib
from m6anet_amd.engine import M6ANetEngine

pytestmark = pytest.mark.gpu
FILL = 7.0


@pytest.fixture(scope="module")
def eng(weights):
    e = M6ANetEngine(weights=weights["hct116"], device=0)
    yield e
    e.close()


def run(eng, pointers, items):
    """p [len(items)] of one call on raw addresses, the sentinels checked and taken off"""
    n, m, h = KE.arrays(items)
    count = len(items)
    if pointers == "host":
        p = np.full(count + 2, FILL)
        eng.ks_exact_ptrs(n.ctypes.data, m.ctypes.data, h.ctypes.data, count, p.ctypes.data + 8)
        got = p
    else:
        import torch
        dn, dm, dh = (torch.from_numpy(x).cuda() for x in (n, m, h))
        p = torch.full((count + 2,), FILL, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        eng.ks_exact_ptrs(dn.data_ptr(), dm.data_ptr(), dh.data_ptr(), count, p.data_ptr() + 8)
        eng.sync()
        got = p.cpu().numpy()
    assert got[0] == FILL and got[-1] == FILL
    return got[1:-1]


def check(eng, pointers, items):
    got, want = run(eng, pointers, items), KE.host(items)
    bad = [(it, g, w) for it, g, w in zip(items, got, want) if not KE.same_bits([g], [w])]
    assert not bad, (len(bad), bad[:5])
    return got


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_crossed_sizes(eng, pointers):
    items = KE.cross()
    got = check(eng, pointers, items)
    n, m, h = KE.arrays(items)
    assert np.isnan(got[h < 0]).all() and (got[h == 0] == 1.0).all() and (got[h > n * m] == 0.0).all() and not np.isnan(got[h >= 0]).any()


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_named_items(eng, pointers):
    got = dict(zip(KE.SPECIAL, check(eng, pointers, list(KE.SPECIAL.values()))))
    assert sorted(k for k, v in got.items() if np.isnan(v)) == sorted(KE.NAN)
    assert got["a band narrower than one cell"] == 1.0 and got["a band that covers the grid"] == 0.0
    assert 0.0 < got["a subnormal result"] < 2.0 ** -1022 and got["a zero result"] == 0.0   # float64 subnormals are kept
    assert 0.01 < got["the cell cap"] < 0.99 and 0.01 < got["the short cap"] < 0.99


def test_bags_swapped_give_the_same_bits(eng):
    items = [it for it in KE.cross() if it[0] != it[1]] + [it for name, it in KE.SPECIAL.items() if it[0] != it[1] and "int64" not in name]
    assert KE.same_bits(run(eng, "device", items), run(eng, "device", [(m, n, h) for n, m, h in items]))


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_one_launch_of_mixed_items_past_the_grid(eng, pointers):
    import torch
    count = 4 * 64 * torch.cuda.get_device_properties(0).multi_processor_count + 4 * 97      # four items per block: no grid covers them in one pass
    items = KE.mixed(count)
    cells = np.array([n * m for n, m, _ in items[:8]])
    assert cells[1] > 40 * np.delete(cells, 1).max()             # a block's second wavefront against its neighbours
    check(eng, pointers, items)


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_engine_method_on_arrays_and_tensors(eng, pointers):
    items = KE.cross()[:140]
    n, m, h = (x.reshape(20, 7) for x in KE.arrays(items))
    if pointers == "host":
        got = eng.ks_exact(n, m, h)
    else:
        import torch
        resident = [torch.from_numpy(x).cuda() for x in (n, m, h)]      # held until the queued call has run
        torch.cuda.synchronize()
        got = eng.ks_exact(*resident)
        eng.sync()
        got = got.cpu().numpy()
    assert got.shape == (20, 7) and KE.same_bits(got.ravel(), KE.host(items))
    with pytest.raises(ValueError):
        eng.ks_exact(n, m, h[:10])


def test_no_items_null_and_mixed_pointers(eng):
    import torch
    f = eng._L.m6a_ks_exact
    n, m, h = KE.arrays([(20, 20, 100), (5, 7, 3)])
    p = np.full(2, FILL)
    dn, dp = torch.from_numpy(n).cuda(), torch.full((2,), FILL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert f(eng._h, None, None, None, 0, None) == 0 and f(eng._h, n.ctypes.data, m.ctypes.data, h.ctypes.data, 0, p.ctypes.data) == 0
    for args in ((n.ctypes.data, m.ctypes.data, h.ctypes.data, 2, None), (None, m.ctypes.data, h.ctypes.data, 2, p.ctypes.data),
                 (n.ctypes.data, m.ctypes.data, h.ctypes.data, -1, p.ctypes.data),
                 (dn.data_ptr(), m.ctypes.data, h.ctypes.data, 2, p.ctypes.data),       # a mixture of host and device pointers
                 (n.ctypes.data, m.ctypes.data, h.ctypes.data, 2, dp.data_ptr())):
        with pytest.raises(_lib.M6AError) as e:
            eng.ks_exact_ptrs(*args)
        assert e.value.code == -1                                # M6A_EINVAL
    eng.sync()
    assert (p == FILL).all() and (dp.cpu().numpy() == FILL).all()
    assert KE.same_bits(run(eng, "host", [(20, 20, 100)]), KE.host([(20, 20, 100)]))     # the context goes on
