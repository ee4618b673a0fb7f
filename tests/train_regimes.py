"""The case tables of tests/test_gpu_train_regimes.py (the kernels) and tests/test_train_regimes.py (the yardstick's own conditions,
without a GPU): the two read the same shapes, seeds and weights from here, so they cannot drift.

A case is (weights, batch); a family is the cases of one (weights kind, B, bag) over its seeds, pooled as train_torch.hold pools.
Batches are test_gpu_train.make_batch's with test_step_shapes' seed rule, 1000 B + 10 bag + seed.
"""
import numpy as np

import weight_families as WF

SEEDS = (11, 12, 13, 14)                                  # test_gpu_train.SEEDS
HCT = "HCT116_RNA002"

# ---- under the given-s bar (train_torch.py): (weights kind, B, bag) -----------------------------------------------------------------
GIVEN_S = [
    # the low end: labelled sites with s near 0; at 500 and 8200 sites some s are exactly 0 in float32
    ("HCT116", 2, 1), ("HCT116", 64, 1), ("HCT116", 500, 1), ("HCT116", 130, 2), ("HCT116", 7, 5),
    # where `train` starts: a fresh blob, 1 - s about 1e-6 at 20 reads
    ("init", 64, 20), ("init", 13, 20), ("init", 16, 5),
    # the high end test_gpu_train.condition refuses: 1 - s falls to 1e-4 .. 3e-3
    ("HCT116", 5, 63), ("HCT116", 130, 64),
    # 129 waves, chunks of 64 reads, the embedding fold over 8 200 bags
    ("HCT116", 8200, 1),
    # 21 and 32 bags per wave
    ("HCT116", 45, 3), ("HCT116", 70, 2),
]
WEIGHT_FAMILIES = ("fresh", "trained_like", "perturbed", "gamma_signs", "large", "big_embedding")
WEIGHT_SHAPES = [(13, 20), (7, 5)]
GIVEN_S += [(f, B, bag) for f in WEIGHT_FAMILIES for B, bag in WEIGHT_SHAPES]

# the two cases that say why the given-s bar exists: under the plain bar E_ref is above 1e-3 of the gradient
PLAIN_BAR_IS_EMPTY = [("init", 64, 20), ("HCT116", 500, 1)]

# ---- under the plain bar with test_gpu_train.condition(), HCT116 --------------------------------------------------------------------
# chunk = max(32, round_up_32(ceil(N / 256))) reads: beyond N = 8 192 a chunk is more than one 32-read tile
BEYOND_ONE_TILE = [(410, 20),                             # chunks of 64, 129 of them, the last one 8 reads
                   (412, 20),                             # chunks of 64, the last one a full tile and 16 reads
                   (821, 20),                             # chunks of 96, 172 of them, the last one 4 reads
                   (260, 33)]                             # chunks of 64, a bag per wave with idle lanes
# bags per wave: 1 with idle lanes, 2 with none, 3, 2, 21, 32; every one with a short last wave, (6, 33) and (9, 2x) with a last
# block of fewer than 4 waves
BAG_GEOMETRIES = [(6, 33), (7, 32), (9, 21), (9, 22), (45, 3), (70, 2)]
CHANGING_SHAPES = [(3, 20), (412, 20), (7, 5), (6, 33)]  # one trainer, in this order


def seeds_for(B, bag):
    return SEEDS if B * bag <= 16000 else SEEDS[:2]


def batch_seed(B, bag, seed):
    return 1000 * B + 10 * bag + seed


def weights(kind, seed):
    """seed: the case's seed of SEEDS.  A weight family alternates its two seeds of weight_families.SEEDS over them."""
    from m6anet_amd.engine import init_weights, load_weights
    if kind == "HCT116":
        return load_weights(HCT)
    if kind == "init":
        return init_weights(seed)
    return WF.blob(kind, WF.SEEDS[kind][SEEDS.index(seed) % len(WF.SEEDS[kind])])


def cases(bundled, kind, B, bag):
    """-> [(weights, batch)], one per seed of the family."""
    from test_gpu_train import make_batch
    return [(weights(kind, s), make_batch(bundled, B, bag, batch_seed(B, bag, s))) for s in seeds_for(B, bag)]


def name(kind, B, bag):
    return "given s: %s %dx%d" % (kind, B, bag)


def chunking(N):
    """-> (chunk reads, chunks, reads of the last chunk), as m6a_train.hip's queue_step cuts a batch."""
    chunk = max(32, -(-(-(-N // 256)) // 32) * 32)
    n = -(-N // chunk)
    return chunk, n, N - (n - 1) * chunk
