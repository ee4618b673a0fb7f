"""What level 2 of the BGZF writer promises of a vector of code lengths (include/m6a.h; m6anet_amd/csrc/m6a_deflate.h code_lengths),
in plain Python: the limit, Kraft completeness with the two exceptions of RFC 1951, and what a Huffman code of the same counts costs."""
import heapq
from fractions import Fraction


def check(freq, lengths, limit):
    """lengths is a valid answer for freq: a used symbol has a length of 1..limit and an unused one 0; a single used symbol has
    length 1; no used symbol gives no code at all; otherwise the Kraft sum is exactly 1"""
    assert len(lengths) == len(freq)
    used = [s for s, f in enumerate(freq) if f]
    assert all((lengths[s] > 0) == (freq[s] > 0) for s in range(len(freq))), (freq, lengths)
    assert all(0 <= n <= limit for n in lengths), (lengths, limit)
    if len(used) == 0:
        return
    if len(used) == 1:
        assert lengths[used[0]] == 1, lengths
        return
    assert sum(Fraction(1, 1 << lengths[s]) for s in used) == 1, (freq, lengths)


def cost(freq, lengths):
    return sum(f * n for f, n in zip(freq, lengths))


def huffman(freq):
    """(the bits a Huffman code of freq spends, the depth of its deepest leaf); one used symbol costs a bit each time.  Among the
    optimal trees the depth is that of the one that merges the shallowest of equal weights first, the least deep of them."""
    used = [f for f in freq if f]
    if len(used) < 2:
        return sum(used), len(used)
    heap = [(f, 0) for f in used]
    heapq.heapify(heap)
    total = 0
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        total += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return total, heap[0][1]
