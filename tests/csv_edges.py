"""Seeded arrays at the edges of the CSV writers, as keyword arguments of NativeSites.from_arrays + write_csv, of
csv_statement.texts() and of _io.csv_format(): the set tests/test_csv_statement.py holds the host writer to and
tests/test_gpu_csv_device.py holds the device writer to."""
import numpy as np

KMERS = (b"GGACT", b"AAACA", b"TGACC", b"GAACT")
TIES_EVEN = (1, 5, 77773)                       # m / 2^17 for odd m is an exact tie at the 16th decimal: these keep the even digit,
TIES_UP = (3, 7, 99999, 131071)                 # these round up


def f32_bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def f64_bits(u):
    return np.array([u], np.uint64).view(np.float64)[0]


def prob32():
    one = np.float32(1)
    v = [np.float32(0), f32_bits(1), one, np.nextafter(one, np.float32(0)), np.float32(0.5), f32_bits(0x7fc00000), f32_bits(0xffc00000),
         f32_bits(0x7f800001), f32_bits(0x007fffff), f32_bits(0x00800000), np.float32(1.9999999)]
    v += [np.float32(m / 2.0 ** 17) for m in TIES_EVEN + TIES_UP]
    assert all(float(x) == m / 2.0 ** 17 for x, m in zip(v[-7:], TIES_EVEN + TIES_UP))
    return v


def ratio64():
    v = [0.0, 5e-324, 1.0, 0.5, 1e-300, 5e-17, 2.0 ** -55, 1.9999999999999998, float(np.nextafter(1.0, 0.0)), f64_bits(0x7ff8000000000000),
         f64_bits(0xfff8000000000000), f64_bits(0x7ff0000000000001), 4.9999999999999999e-17, 5.0000000000000001e-17]
    v += [k / n for n in (3, 7, 20, 99, 1000) for k in (1, 2, n - 1)]
    v += [m / 2.0 ** 17 for m in TIES_EVEN + TIES_UP] + [1.0 + m / 2.0 ** 17 for m in TIES_EVEN + TIES_UP]
    return [np.float64(x) for x in v]


def digit_edges(top):
    """0, 9, 10, 99, 100, ... every digit count up to `top`'s, and `top` itself"""
    v, p = [0], 10
    while p <= top:
        v += [p - 1, p]
        p *= 10
    return v + [top]


def build(rng, names, bags, positions, ids_pool, n_rep=1, reps=None, specials=True):
    S = len(bags)
    off = np.zeros(S + 1, np.int64)
    off[1:] = np.cumsum(bags)
    R = int(off[-1])
    tx_off = np.zeros(len(names) + 1, np.int64)
    tx_off[1:] = np.cumsum([len(n) for n in names])
    p32, r64 = (prob32(), ratio64()) if specials else ([], [])
    read_prob = rng.random(R).astype(np.float32)
    site_prob = rng.random(S).astype(np.float32)
    mod_ratio = (rng.integers(0, 1000, S) / 1000.0 + rng.integers(0, 2, S)).astype(np.float64)
    for k, x in enumerate(p32):                          # specials first in the first bag, then spread
        read_prob[(k * 7919) % R if k >= len(p32) // 2 else k] = x
        site_prob[k % S] = x
    for k, x in enumerate(r64):
        mod_ratio[k % S] = x
    ids = rng.integers(0, 10 ** 7, R).astype(np.float64)
    for k, x in enumerate(ids_pool):
        ids[(k * 104729) % R if k % 2 else k] = float(x)
    a = dict(off=off, tx_pos=np.array([positions[i % len(positions)] for i in range(S)], np.int64), tx_blob=b"".join(names), tx_off=tx_off,
             site_tx=np.array([i % len(names) for i in range(S)], np.uint32),
             kmer5=np.frombuffer(b"".join(KMERS[i % 4] for i in range(S)), np.uint8).reshape(S, 5).copy(), read_ids=ids,
             read_prob=read_prob, site_prob=site_prob, mod_ratio=mod_ratio)
    if n_rep > 1:
        a.update(n_rep=n_rep, read_rep=np.array([reps[int(x)] for x in rng.integers(0, len(reps), R)], np.int32))
    return a


def cases(seed=5):
    """name -> arrays.  `main`: every edge of the issue's list in one job; `rep`: the same with replicate numbers 0, 9 and 10;
    `empty`, `one`: S = 0 and S = 1; `wide`: 2^20 + reads so that the scans span several workgroups."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTNENST0123456789._|-", np.uint8)
    names = [bytes(letters[rng.integers(0, len(letters), n)]) for n in (1, 2, 3, 4, 255, 4096, 15, 18, 9000, 5, 6, 7)]
    positions = digit_edges(2 ** 63 - 1) + [-1, -10, -2 ** 63, 12345]
    ids_pool = digit_edges(10 ** 15 - 1)
    bags = [20, 99, 100, 1003, 21, 64, 65, 63, 128, 1] + [int(x) for x in rng.integers(20, 90, 50)]
    out = {"main": build(rng, names, bags, positions, ids_pool),
           "rep": build(rng, names, bags, positions, ids_pool, n_rep=11, reps=(0, 9, 10)),
           "empty": build(rng, names[:1], [], positions, [], specials=False),
           "one": build(rng, [b"T"], [20], [7], [3]),
           "wide": build(rng, [b"ENST%011d.%d" % (t, t % 9) for t in range(300)], [int(x) for x in rng.integers(20, 700, 3000)],
                         [int(x) for x in rng.integers(0, 10 ** 5, 997)], ids_pool)}
    assert int(out["wide"]["off"][-1]) >= 2 ** 20 and len(out["empty"]["tx_pos"]) == 0
    return out


def declined_cases(seed=6):
    """name -> (arrays, how many values csv_statement.declines() must count): one array per class of declined value, one such value"""
    rng = np.random.default_rng(seed)
    out = {}
    spots = {"read_prob_negative": ("read_prob", np.float32(-0.25)), "read_prob_minus_zero": ("read_prob", np.float32(-0.0)),
             "read_prob_two": ("read_prob", np.float32(2.0)), "site_prob_negative": ("site_prob", np.float32(-1e-30)),
             "site_prob_large": ("site_prob", np.float32(3e38)), "mod_ratio_negative": ("mod_ratio", -0.0),
             "mod_ratio_two": ("mod_ratio", 2.0), "mod_ratio_large": ("mod_ratio", 1e300), "id_fraction": ("read_ids", 12.5),
             "id_negative": ("read_ids", -3.0), "id_minus_zero": ("read_ids", -0.0), "id_1e15": ("read_ids", 1e15), "id_nan": ("read_ids", float("nan")),
             "id_inf": ("read_ids", float("inf"))}
    for k, (name, (field, value)) in enumerate(sorted(spots.items())):
        a = build(rng, [b"TX1", b"TX22"], [20, 30, 25], [5, 50, 500], [1, 2, 3], specials=False,
                  **(dict(n_rep=2, reps=(0, 1)) if k % 2 else {}))
        a[field][len(a[field]) // 2] = value
        out[name] = (a, 1)
    return out
