#!/usr/bin/env python3
"""Where a tile's wall time goes inside enc_site16_kernel, from the kernel's own clock: a diagnostic build (never the product) stamps
s_memtime at ten points of 16 consecutive tiles of EVERY wave, with the wave's hardware slot, so the two waves that share a SIMD can
be laid side by side.  The stamp buffer, its reader and the ten stamp points are not in m6a_kernels.hip: stamps() below inserts them
into a copy (tools/variant_build.py), on top of encoder_ab.py's priority edits for stamps_noprio / stamps_body3_epi0.  Six of the ten
points lie inside unit_tile_loop and store_prob_as_reference, which enc_site16_kernel shares with the other encoder kernels: the copy
gives those two a defaulted extra functor (a no-op for every other caller) and enc_site16_kernel passes the stamp.

    python tools/encoder_timeline.py --build     (here: cross-compiles tools/ko/libm6a_ab_stamps.so, which travels to the GPU box)
    python tools/encoder_timeline.py             (GPU box: one JSON object)

Sections of a tile (stamp i -> i+1) and the MFMAs this wave issues in each:
  0-1  link0 (scalar loads of off[]) + layer 1 of unit tile 0                      8
  1-2  layer 1 of unit tile 1, link1 (x loads), batch norm + layer 2 of unit tile 0 24
  2-3  layer 1 of unit tile 2, link2, batch norm + layer 2 of unit tile 1          24
  3-4  layer 1 of unit tile 3, batch norm + layer 2 of unit tile 2                 24
  4-5  layer 1 of unit tile 4, link3 (ds_bpermute), batch norm + layer 2 of unit tile 3   24
  5-6  batch norm + layer 2 of unit tile 4 (12 hidden units)                       12
  6-7  32 -> 1 layer (relu, products, butterfly, two exchanges between the lane halves)   0
  7-8  sigmoid (Sleef expf, IEEE divide) + the store                                0
  8-9  site base for the next tile (shuffle + readfirstlane), feature registers handed over   0
  9-0' loop back (in the stamped tiles also: lane 0 stores the ten stamps)          0
With two waves per SIMD taking turns on the matrix pipe, a section with n MFMAs lasts >= 128 n cycles while the partner is in its body too.

No longer built: stamps_phase, stamps_phase_noprio, stamps_phase_body3_epi0, stamps_phase_eqprio (the second workgroup of a CU started half
a tile late: an `#ifdef M6A_AB_PHASE` branch of the kernel source itself).  Their results are in profiles/r06_encoder_timeline.json; the last
commit that can build them is 53ba79eec7177618b64cf16fbcc604bc27170bd0.
"""
import ctypes
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from encoder_ab import lib, no_prio, prio
from variant_build import REPO, build, swap, within

sys.path.insert(0, REPO)
TILES, POINTS, FIRST, MAXW = 16, 10, 100, 4096

STAMP_STATE = """// Diagnostic build only: every wave of enc_site16_kernel stamps s_memtime at ten points of each of %(TILES)d consecutive tiles from its
// %(FIRST)d-th on, with its hardware slot (HW_ID, XCC_ID).  The stamps are scalar instructions with no wait; lane 0 stores them after the
// last stamp of a tile.
__device__ unsigned long long m6a_ab_stamp_buf[%(MAXW)d][%(TILES)d][%(POINTS)d];
__device__ unsigned m6a_ab_stamp_hw[%(MAXW)d][2];
extern "C" int m6a_ab_read_stamps(unsigned long long *stamps, unsigned *hw)
{
    if (hipMemcpyFromSymbol(stamps, HIP_SYMBOL(m6a_ab_stamp_buf), sizeof(m6a_ab_stamp_buf)) != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(hw, HIP_SYMBOL(m6a_ab_stamp_hw), sizeof(m6a_ab_stamp_hw)) != hipSuccess) return -1;
    return 0;
}
#define M6A_STAMP(k) do { __builtin_amdgcn_sched_barrier(0); ts[k] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
""" % {"TILES": TILES, "POINTS": POINTS, "FIRST": FIRST, "MAXW": MAXW}
STAMP_STORE = """        M6A_STAMP(9);
        {
            const int k = tile - tile0 - %(FIRST)d;
            if (k >= 0 && k < %(TILES)d && sc.wave < %(MAXW)d && lane == 0) {
#pragma unroll
                for (int i = 0; i < %(POINTS)d; i++) m6a_ab_stamp_buf[sc.wave][k][i] = ts[i];
                if (k == 0) {
                    m6a_ab_stamp_hw[sc.wave][0] = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));       // HW_REG_HW_ID
                    m6a_ab_stamp_hw[sc.wave][1] = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11));      // HW_REG_XCC_ID
                }
            }
        }
""" % {"TILES": TILES, "POINTS": POINTS, "FIRST": FIRST, "MAXW": MAXW}
KERNEL = "__global__ __launch_bounds__(256, 2) void enc_site16_kernel(EncArgs a)\n"
LOOP = "template <class Layer1, class Links>\n__device__ __forceinline__ void unit_tile_loop("
EPILOGUE = "__device__ __forceinline__ void store_prob_as_reference("
PASS_STAMP = ", [&](int k) { M6A_STAMP(k); });\n"


def stamps(s):
    """The stamp buffer and its reader in front of enc_site16_kernel, the ten stamp points and the store into its tile loop."""
    def hook(fn, *points):
        """A shared piece calls stamp(k) behind each given line; stamp is a trailing functor that defaults to nothing."""
        fn = swap(fn, ")\n{\n", ", Stamp &&stamp = Stamp())\n{\n")
        for line, k in points:
            fn = swap(fn, line, line + line[:len(line) - len(line.lstrip())] + "stamp(%s);\n" % k)
        return fn
    s = within(s, LOOP, "\n}\n", lambda fn: hook(fn, ("    layer1(0, h1a);\n", "1"), ("        if (m == 4) layer2_with_bn<4>(acc2, cur, w2, bnq, bn_half);\n", "2 + m")))
    s = swap(s, LOOP, "struct NoStamp { __device__ void operator()(int) const {} };\n" + LOOP.replace("class Links>", "class Links, class Stamp = NoStamp>"))
    s = within(s, EPILOGUE, "\n}\n", lambda fn: hook(fn, ("    const float z = gemv32_as_mkl(acc2, w3, half) + b3;\n", "7")))
    s = swap(s, EPILOGUE, "template <class Stamp = NoStamp> " + EPILOGUE)

    def tile_loop(k):
        k = swap(k, "        int reln, kidn;\n        sc.link0(s_base, o);\n", "        int reln, kidn;\n        unsigned long long ts[%d];\n        M6A_STAMP(0);\n        sc.link0(s_base, o);\n" % POINTS)
        k = swap(k, "        });\n        tile_epilogue_priority();\n", "        }" + PASS_STAMP + "        tile_epilogue_priority();\n")          # stamps 1 .. 6
        k = swap(k, "a.read_prob + (int64_t)tile * 32 + col);\n", "a.read_prob + (int64_t)tile * 32 + col" + PASS_STAMP + "        M6A_STAMP(8);\n")       # 7, 8
        line = "        for (int i = 0; i < 8; i++) f[i] = fn[i];\n"
        return swap(k, line, line + STAMP_STORE)
    s = within(s, KERNEL, "\n}\n", tile_loop)
    return swap(s, KERNEL, STAMP_STATE + KERNEL)


VARIANTS = {"stamps": stamps, "stamps_noprio": lambda s: stamps(no_prio(s)), "stamps_body3_epi0": lambda s: stamps(prio(3, 0)(s))}
MFMA = [8, 24, 24, 24, 24, 12, 0, 0, 0, 0]
NAMES = ["link0 + L1(0)", "L1(1) + link1 + BN/L2(0)", "L1(2) + link2 + BN/L2(1)", "L1(3) + BN/L2(2)", "L1(4) + link3 + BN/L2(3)", "BN/L2(4)",
         "32->1 layer", "sigmoid + store", "site base + hand-over", "loop back (+ stamp stores)"]


def med(v):
    v = sorted(v)
    return v[len(v) // 2] if v else None


def main():
    if "--build" in sys.argv:
        build("m6a_kernels.hip", VARIANTS, "libm6a_ab_%s.so")
        return
    if "--one" not in sys.argv:
        out = {}
        for name in VARIANTS:
            if not os.path.exists(lib(name)):
                continue
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"], env=dict(os.environ, M6A_HIP_LIB=lib(name)), capture_output=True, text=True, timeout=600)
            try:
                out[name] = json.loads(o.stdout.strip().splitlines()[-1])
            except (ValueError, IndexError):
                out[name] = {"error": (o.stderr or o.stdout)[-400:]}
        print(json.dumps(out))
        return
    LIB = os.environ["M6A_HIP_LIB"]
    import numpy as np
    import torch
    from m6anet_amd import synthetic
    from m6anet_amd.engine import M6ANetEngine, load_weights
    eng = M6ANetEngine(weights=load_weights("HCT116_RNA002"))
    d = synthetic.make_sites(1_000_000, 20, seed=20250328)
    X, km, off = (torch.from_numpy(d[k]).cuda() for k in ("X", "site_kmers", "off"))
    rp = torch.empty(int(d["off"][-1]), dtype=torch.float32, device="cuda")
    eng.set_encoder_variant(0)
    for _ in range(4):
        eng.get_read_probability(X, km, off, out=rp)
    eng.sync()
    eng.profile("encoder")
    for _ in range(20):
        eng.get_read_probability(X, km, off, out=rp)
    ms, n = eng.profile_read(0)
    eng.profile(False)
    assert eng.last_encoder_kernel == "enc_site16_kernel"
    dll = ctypes.CDLL(LIB)
    st = np.zeros((MAXW, TILES, POINTS), dtype=np.uint64)
    hw = np.zeros((MAXW, 2), dtype=np.uint32)
    rc = dll.m6a_ab_read_stamps(st.ctypes.data_as(ctypes.c_void_p), hw.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    live = np.nonzero(st[:, 0, 0])[0]
    st = st.astype(np.int64)
    # sections
    sec = []
    for i in range(POINTS):
        if i < POINTS - 1:
            dur = (st[live, :, i + 1] - st[live, :, i]).ravel()
        else:
            dur = (st[live, 1:, 0] - st[live, :-1, POINTS - 1]).ravel()
        sec.append({"section": "%d-%s" % (i, i + 1 if i < POINTS - 1 else "0'"), "what": NAMES[i], "mfma": MFMA[i], "median_cycles": float(np.median(dur)),
                    "mean_cycles": float(dur.mean()), "p10": float(np.percentile(dur, 10)), "p90": float(np.percentile(dur, 90)),
                    "cycles_per_own_mfma": float(np.median(dur)) / MFMA[i] if MFMA[i] else None})
    tile = (st[live, 1:, 0] - st[live, :-1, 0]).ravel()
    # pairs: waves in the same (xcc, se, sh, cu, simd)
    key = {}
    for w in live:
        h, x = int(hw[w, 0]), int(hw[w, 1]) & 0xf
        k = (x, (h >> 13) & 7, (h >> 12) & 1, (h >> 8) & 0xf, (h >> 4) & 3)
        key.setdefault(k, []).append(int(w))
    pairs = [v for v in key.values() if len(v) == 2]
    both_epi, a_epi_only, phase, idle_model = [], [], [], []
    for a, b in pairs:
        t0 = max(st[a, 0, 0], st[b, 0, 0])
        t1 = min(st[a, TILES - 1, 9], st[b, TILES - 1, 9])
        if t1 <= t0:
            continue
        # intervals in which a wave issues no MFMA: stamp 6 (end of the body) .. the next tile's stamp 0
        def gaps(w):
            g = [(st[w, k, 6], st[w, k + 1, 0]) for k in range(TILES - 1)]
            return [(max(s, t0), min(e, t1)) for s, e in g if min(e, t1) > max(s, t0)]
        ga, gb = gaps(a), gaps(b)
        la, lb = sum(e - s for s, e in ga), sum(e - s for s, e in gb)
        ov = sum(max(0, min(e1, e2) - max(s1, s2)) for s1, e1 in ga for s2, e2 in gb)
        span = float(t1 - t0)
        both_epi.append(ov / span)
        a_epi_only.append((la + lb - 2 * ov) / span)
        per = float(np.median(st[a, 1:, 0] - st[a, :-1, 0]))
        phase.append(float(((st[b, 8, 0] - st[a, 8, 0]) % per) / per))
    ex = None
    if pairs:
        a, b = pairs[len(pairs) // 2]
        t0 = int(min(st[a, 4, 0], st[b, 4, 0]))
        ex = {"waves": [a, b], "stamps_minus_t0": {"a": (st[a, 4:8] - t0).tolist(), "b": (st[b, 4:8] - t0).tolist()}}
    out = {"what": "enc_site16_kernel, 20 M reads (1 M sites x 20), s_memtime stamps of tiles %d..%d of every wave (diagnostic build)" % (FIRST, FIRST + TILES - 1),
           "kernel_ms": ms / n, "waves": int(len(live)), "tile_cycles_median": float(np.median(tile)), "tile_cycles_mean": float(tile.mean()),
           "mfma_cycles_per_tile_of_both_waves": 2 * 116 * 64,
           "matrix_pipe_busy_from_stamps": 2 * 116 * 64 / float(np.median(tile)),
           "sections": sec,
           "pairs": {"simd_slots_with_two_stamped_waves": len(pairs), "slots_seen": len(key),
                     "share_of_time_both_waves_outside_their_mfma_body": med(both_epi),
                     "share_of_time_exactly_one_wave_outside_its_body": med(a_epi_only),
                     "hw_wave_id_of_the_two": [[int(hw[a, 0]) & 0xf, int(hw[b, 0]) & 0xf] for a, b in pairs[:8]],
                     "phase_of_partner_tile_start_in_own_tile_deciles": [float(np.percentile(phase, q)) for q in range(0, 101, 10)] if phase else None},
           "example_pair": ex}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
