"""Variant builds of the library for the A/B and knock-out tools: the product source stays as it ships, a variant is a text edit of a
COPY of one source file (a function str -> str whose anchors are asserted, so an edit that no longer applies fails loudly), written
to tools/ko/ and compiled from there against the objects of the untouched sources.  tools/ko/ is git-ignored and travels to the GPU box.
"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "m6anet_amd", "csrc")
KO = os.path.join(HERE, "ko")


def sub(pattern, repl, s, count=1, flags=0):
    """re.sub that must match."""
    out, n = re.subn(pattern, repl, s, count=count, flags=flags)
    assert n >= 1, pattern
    return out


def swap(s, old, new, count=1):
    """str.replace of a literal that must occur exactly `count` times."""
    assert s.count(old) == count, (s.count(old), old)
    return s.replace(old, new)


def within(s, start, end, fn):
    """fn applied to the part of s from the (one) literal `start` up to the next `end`: an anchor need only be unique in there."""
    assert s.count(start) == 1, start
    a = s.index(start)
    b = s.index(end, a + len(start))
    return s[:a] + fn(s[a:b]) + s[b:]


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def build(src_name, variants, lib_fmt, only=None):
    """variants: {name: edit of src_name's text}; writes tools/ko/<lib_fmt % name>, the library with that one source edited."""
    sys.path.insert(0, REPO)
    from m6anet_amd.build import SOURCES
    os.makedirs(KO, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-w",
             '-DM6A_MT_JUMP_PATH="%s"' % os.path.join(REPO, "m6anet_amd", "assets", "mt19937_jump.bin"),
             "-I" + os.path.join(REPO, "include"), "-I" + CSRC]
    text = source(src_name)
    edited = {name: fn(text) for name, fn in variants.items() if only is None or name in only}       # every anchor checked before the first compile
    objs = []
    for f in [x for x in SOURCES if x != src_name]:
        o = os.path.join(KO, "asis_" + f.replace(".hip", ".o"))
        if not os.path.exists(o) or os.path.getmtime(o) < os.path.getmtime(os.path.join(CSRC, f)):
            subprocess.check_call([hipcc] + flags + ["-c", os.path.join(CSRC, f), "-o", o])
        objs.append(o)
    for name, body in edited.items():
        lib = os.path.join(KO, lib_fmt % name)
        p = lib[:-3] + "_" + src_name
        with open(p, "w") as f:
            f.write(body)
        o = p.replace(".hip", ".o")
        subprocess.check_call([hipcc] + flags + ["-c", p, "-o", o])
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + [o, "-o", lib])
        print("built", lib)
