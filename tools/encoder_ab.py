#!/usr/bin/env python3
"""A/B of encoder-kernel builds on the bench shape (20 M reads): HIP-event time per launch of the two scalar-chain kernels, per build,
legs interleaved A B C A B C ... so clock drift hits every build alike.

    python tools/encoder_ab.py --build [only=a,b]   (here: cross-compiles the variants into tools/ko/, which travels to the GPU box)
    python tools/encoder_ab.py [legs] [only=a,b]    (GPU box: one JSON line)

m6a_kernels.hip holds the product and nothing else.  A variant is an edit of a COPY of it (a function str -> str with asserted anchors,
tools/variant_build.py), one or two lines each:
  base               the product
  links_abc          enc_site16_kernel: links 1 / 2 / 3 of the input chain at m = a / b / c of the unit-tile loop instead of 1 / 2 / 3 (rounds 2-6a: 0 / 1 / 3; same bits)
  bn_block2 / 8      batch norm woven in blocks of 2 / 8 hidden units instead of 4 (same bits)
  no_prio            the product WITHOUT its wave-priority split (s_setprio 0 through a tile's MFMA body, 3 through its epilogue; same bits)
  prio_body3_epi0    the round's first split, the other way round (body 3, epilogue 0); p01 / p13 / p23: body / epilogue priorities 0/1, 1/3, 2/3
  no_epilogue        knock-out, WRONG RESULTS, timing only: the 32 -> 1 layer + sigmoid removed from enc_site16_kernel (what the epilogue costs in
                     place = the most that hiding it under the next tile's MFMAs could buy)

Variants of round 6 that are no longer built.  They were `#ifdef M6A_AB_*` branches of the kernel source itself; the last commit that can build them
(python tools/encoder_ab.py --build there) is 53ba79eec7177618b64cf16fbcc604bc27170bd0.  Where each result is kept (profiles/):
  w3 (three waves per SIMD, layer 2's A operands from LDS)          r06_encoder_ab_three_waves.json
  l2_first (layer 2 in front of the next unit tile's layer 1)       r06_encoder_ab_schedule.json
  addr64 (link1's loads with 64-bit VALU address arithmetic)        r06_encoder_ab_addr32.json
  no_bn, no_links, no_bn_no_epilogue, no_bn_no_epilogue_no_links    r06_encoder_ab_knockouts.json (wrong results, timing only)
  bn_pk (batch norm two units per v_pk_fma_f32)                     r06_encoder_ab_priority_and_packed_bn.json
  prio_block_valu_low / _high (priorities inside the body)          r06_encoder_ab_prio_block.json
  p03_bn2, p13_bn0                                                  r06_encoder_ab_prio_sweep.json
  phase, phase_hwid (second wave of a SIMD half a tile late)        r06_encoder_ab_phase.json
  no_epilogue_phase, _phase_quarter, _phase_eighth                  r06_encoder_ab_no_epilogue_phase.json
  prev (by then the same build as base)                             r06_encoder_ab_scalar_site_advance.json
  csite_scalar_fma, csite_pin (link3's packed fmas plain / pinned)  no file: the numbers are in HISTORY.md, round 6, "A/B builds of the encoder"
"""
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from variant_build import KO, REPO, build, swap, within

sys.path.insert(0, REPO)


SITE16 = "__global__ __launch_bounds__(256, 2) void enc_site16_kernel(EncArgs a)\n"


def in_site16(s, fn):
    """fn applied to the text of enc_site16_kernel alone: the pieces it shares with the other encoder kernels are out of reach."""
    return within(s, SITE16, "\n}\n", fn)


def links(a, b, c):
    def f(k):
        k = swap(k, "if (m == 1) sc.link1(tn, s_base, o, reln, kidn, fn);", "if (m == %d) sc.link1(tn, s_base, o, reln, kidn, fn);" % a)
        k = swap(k, "if (m == 2) sc.link2(kidn, evn);", "if (m == %d) sc.link2(kidn, evn);" % b)
        return swap(k, "if (m == 3) link3(evn, reln, fn);", "if (m == %d) link3(evn, reln, fn);" % c)
    return lambda s: in_site16(s, f)


def prio(body, epi):
    """Wave priority through a tile's MFMA body / its epilogue (the product: 0 / 3), in all three encoder kernels."""
    def f(s):
        s = swap(s, "void tile_body_priority()\n{\n    __builtin_amdgcn_s_setprio(0);", "void tile_body_priority()\n{\n    __builtin_amdgcn_s_setprio(%d);" % body)
        return swap(s, "void tile_epilogue_priority()\n{\n    __builtin_amdgcn_s_setprio(3);", "void tile_epilogue_priority()\n{\n    __builtin_amdgcn_s_setprio(%d);" % epi)
    return f


def no_prio(s):
    s = swap(s, "void tile_body_priority()\n{\n    __builtin_amdgcn_s_setprio(0);\n", "void tile_body_priority()\n{\n")
    return swap(s, "void tile_epilogue_priority()\n{\n    __builtin_amdgcn_s_setprio(3);\n", "void tile_epilogue_priority()\n{\n")


def bn_block(n):
    return lambda s: swap(s, "#define BN_BLOCK 4\n", "#define BN_BLOCK %d\n" % n)


def no_epilogue(s):
    """WRONG RESULTS by construction, timing only: enc_site16_kernel stores a sum of two accumulators instead of the probability
    (its call of the shared epilogue is replaced; the epilogue itself, which enc_kernel and enc_repr_kernel use too, stays)."""
    return in_site16(s, lambda k: swap(k, "        store_prob_as_reference(acc2, w3, half, a.b3, col <= sc.lim(tile), a.read_prob + (int64_t)tile * 32 + col);\n",
                                       "        const float p = (acc2[0] + acc2[5]) + w3[0];      // knock-out: WRONG results\n"
                                       "        if (half == 0 && col <= sc.lim(tile)) (a.read_prob + (int64_t)tile * 32)[col] = p;\n"))


VARIANTS = {"base": lambda s: s, "no_prio": no_prio, "p01": prio(0, 1), "p13": prio(1, 3), "p23": prio(2, 3), "prio_body3_epi0": prio(3, 0),
            "links_013": links(0, 1, 3), "links_012": links(0, 1, 2), "links_024": links(0, 2, 4), "links_124": links(1, 2, 4), "links_014": links(0, 1, 4),
            "links_234": links(2, 3, 4), "links_134": links(1, 3, 4), "links_034": links(0, 3, 4), "links_023": links(0, 2, 3),
            "bn_block2": bn_block(2), "bn_block8": bn_block(8), "no_epilogue": no_epilogue}


def lib(name):
    return os.path.join(KO, "libm6a_ab_%s.so" % name)


def one(legs_unused):
    import torch
    from m6anet_amd import synthetic
    from m6anet_amd.engine import M6ANetEngine, load_weights
    eng = M6ANetEngine(weights=load_weights("HCT116_RNA002"))
    d = synthetic.make_sites(1_000_000, 20, seed=20250328)
    X, km, off = (torch.from_numpy(d[k]).cuda() for k in ("X", "site_kmers", "off"))
    rp = torch.empty(int(d["off"][-1]), dtype=torch.float32, device="cuda")
    out = {}
    for mode, label in ((0, "enc_site16_kernel"), (2, "enc_csite_kernel"), (3, "enc_kernel")):
        eng.set_encoder_variant(mode)
        for _ in range(5):
            eng.get_read_probability(X, km, off, out=rp)
        eng.sync()
        eng.profile("encoder")
        for _ in range(40):
            eng.get_read_probability(X, km, off, out=rp)
        ms, n = eng.profile_read(0)
        clk = eng.profile_clock(0)
        eng.profile(False)
        assert eng.last_encoder_kernel == label
        out[label] = [round(ms / n, 5), round(clk["ghz"], 4) if clk else None]
    print(json.dumps(out))


def main():
    only = [a[5:].split(",") for a in sys.argv[1:] if a.startswith("only=")]          # only=base,no_prio: build / run just these
    only = only[0] if only else None
    if "--build" in sys.argv:
        build("m6a_kernels.hip", VARIANTS, "libm6a_ab_%s.so", only)
        return
    if "--one" in sys.argv:
        one(0)
        return
    nums = [a for a in sys.argv[1:] if a.isdigit()]
    legs = int(nums[0]) if nums else 4
    names = [n for n in VARIANTS if os.path.exists(lib(n)) and (only is None or n in only)]
    res = {n: {} for n in names}
    for leg in range(legs):
        for n in names:
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"], env=dict(os.environ, M6A_HIP_LIB=lib(n)), capture_output=True, text=True, timeout=600)
            try:
                r = json.loads(o.stdout.strip().splitlines()[-1])
            except (ValueError, IndexError):
                res[n].setdefault("error", []).append((o.stderr or o.stdout)[-300:])
                continue
            for k, v in r.items():
                res[n].setdefault(k, []).append(v)
    summary = {}
    for n, r in res.items():
        summary[n] = {k: {"median_ms": sorted(x[0] for x in v)[len(v) // 2], "ms_of_each_leg": [x[0] for x in v], "ghz_of_each_leg": [x[1] for x in v]}
                      for k, v in r.items() if k != "error"}
        if "error" in r:
            summary[n]["error"] = r["error"]
    print(json.dumps({"legs": legs, "launches_per_leg": 40, "workload": "20 M reads (1 M sites x 20), HCT116", "builds": summary}))


if __name__ == "__main__":
    main()
