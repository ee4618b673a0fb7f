"""The shapes tests/test_ks_core.py (the host core), tests/test_gpu_ks.py and tests/test_gpu_signal_ks.py (the kernels) run m6a_site_ks
and m6a_site_signal_ks on, and what tests/ks_statement.py says of them, computed once per (site of A, site of B) and shared.

The sets are those of tests/ranksum_cases.py and tests/signal_ranksum_cases.py -- bag sizes around the wavefront's chunk of 64 and the
LDS tile of 256 crossed, 3000 x 2500, signed zeros, infinities, NaN in one column or in every column, empty bags, complete separation --
with the pairs that are new here appended to both sides (NEW, NEW_SIGNAL), so every pair list of those modules is a pair list here:
  bimodal against unimodal   the medians are equal and the rank-sum sees nothing (|z| < 1) where ks_d is 0.5
  odd and even               3 reads against 4: one middle, two middles
  zero middles               the two middles are -0.0 and 0.0, and -0.0 twice: the median is +0.0
  infinite middles           the two middles are -inf and +inf: the median is NaN in a defined pair
`scalar` and `signal` below have the same functions: sets, n_sites, want, pair_lists, LISTS."""
import functools

import numpy as np

import ks_statement as KS
import ranksum_cases as RC
import signal_ranksum_cases as SC
from ranksum_cases import same_bits  # noqa: F401  (the comparison the tests use)

f32 = np.float32
GRID_PAIRS = SC.GRID_PAIRS
BIMODAL = np.concatenate([np.linspace(0.0625, 0.125, 30), np.linspace(0.875, 0.9375, 30)]).astype(f32)      # middles 0.125 and 0.875
UNIMODAL = np.concatenate([np.linspace(0.4375, 0.49, 30), [0.5], np.linspace(0.51, 0.5625, 30)]).astype(f32)  # 61 reads, middle 0.5
inf = np.inf
NEW = (
    ("bimodal against unimodal", BIMODAL, UNIMODAL),
    ("odd and even", np.array([0.75, 0.25, 0.5], f32), np.array([0.125, 1.0, 0.25, 0.5], f32)),
    ("zero middles", np.array([1.0, 0.0, -1.0, -0.0], f32), np.array([-0.0, -0.0, -0.0], f32)),
    ("infinite middles", np.array([inf, -inf, -inf, inf], f32), np.array([0.5, inf, -inf], f32)),
)


def _off(bags):
    return np.concatenate([[0], np.cumsum([x.shape[0] for x in bags])]).astype(np.int64)


def _append(values_a, off_a, values_b, off_b, new):
    a, b = [values_a] + [s[1] for s in new], [values_b] + [s[2] for s in new]
    oa = np.concatenate([off_a, off_a[-1] + _off([s[1] for s in new])[1:]])
    ob = np.concatenate([off_b, off_b[-1] + _off([s[2] for s in new])[1:]])
    return np.ascontiguousarray(np.concatenate(a), f32), oa, np.ascontiguousarray(np.concatenate(b), f32), ob


class Cases:
    """one of the two calls: its sets, the statement over them and its pair lists"""

    def __init__(self, base, new, statement, columns):
        self.base, self.new, self.statement, self.columns = base, new, statement, columns
        self._one = {}

    @functools.lru_cache(maxsize=None)
    def sets(self):
        """(values_a, off_a, values_b, off_b, names): names[k] is what special pair k, behind the sized sites, is there for"""
        va, oa, vb, ob, names = self.base.sets()
        return _append(va, oa, vb, ob, self.new) + (tuple(names) + tuple(s[0] for s in self.new),)

    def n_sites(self):
        return self.sets()[1].size - 1

    def site_of(self, name):
        return len(self.base.SIZES) + self.sets()[4].index(name)

    def one(self, i, j):
        if (i, j) not in self._one:
            va, oa, vb, ob, _ = self.sets()
            r = self.statement(va[oa[i]:oa[i + 1]], vb[ob[j]:ob[j + 1]])
            self._one[i, j] = r if self.columns == 1 else tuple([x[f] for x in r] for f in range(4))
        return self._one[i, j]

    def want(self, pair_a=None, pair_b=None):
        """the statement's (d_pos, d_neg, med_a, med_b), each [P] or [P, 9], for a pair list over sets(); None: the identity"""
        S = self.n_sites()
        ia = np.arange(S) if pair_a is None else np.asarray(pair_a)
        ib = np.arange(S) if pair_b is None else np.asarray(pair_b)
        keys, inverse = np.unique(ia * S + ib, return_inverse=True)
        each = [self.one(int(k) // S, int(k) % S) for k in keys]
        shape = (-1,) if self.columns == 1 else (-1, self.columns)
        return tuple(np.array([e[f] for e in each], np.int64 if f < 2 else np.float64).reshape(shape)[inverse.ravel()] for f in range(4))

    @functools.lru_cache(maxsize=None)
    def pair_lists(self):
        """the base module's lists (the sized sites crossed and its special pairs, that backwards, 0, 1, 65 and 4097 drawn pairs), the
        pairs that are new here, and a list of more than GRID_PAIRS pairs drawn from the sites of at most 3 reads, which no grid of the
        launch covers in one pass"""
        out = dict(self.base.pair_lists())
        S0, S = self.base.n_sites(), self.n_sites()
        out["new here"] = (np.arange(S0, S, dtype=np.int64), np.arange(S0, S, dtype=np.int64))
        if "past the grid" not in out:
            _, oa, _, ob, _ = self.sets()
            tiny_a, tiny_b = np.flatnonzero(np.diff(oa) <= 3), np.flatnonzero(np.diff(ob) <= 3)
            rng = np.random.default_rng(3301)
            out["past the grid"] = (rng.choice(tiny_a, GRID_PAIRS + 7).astype(np.int64), rng.choice(tiny_b, GRID_PAIRS + 7).astype(np.int64))
        return out

    def pairs(self, name):
        """(pair_a, pair_b, P) of a list of LISTS; the identity has no index arrays"""
        if name == "identity":
            return None, None, self.n_sites()
        ia, ib = self.pair_lists()[name]
        return ia, ib, ia.size


LISTS = ("crossed and special", "backwards", "0 drawn", "1 drawn", "65 drawn", "4097 drawn", "past the grid", "new here", "identity")


def _signal_new():
    rng = np.random.default_rng(3302)
    sizes = {name: (a.size, b.size) for name, a, b in NEW}
    column = {"bimodal against unimodal": 8, "odd and even": 1, "zero middles": 0, "infinite middles": 6}
    return tuple((name + " in column %d" % column[name], SC.put(SC.rows(rng, sizes[name][0], 0), column[name], a),
                  SC.put(SC.rows(rng, sizes[name][1], 1), column[name], b)) for name, a, b in NEW)


scalar = Cases(RC, NEW, KS.pair, 1)
signal = Cases(SC, _signal_new(), KS.signal_pair, KS.N_COLUMNS)
