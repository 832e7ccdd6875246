"""The tree fold of MPIX_Reduce_local_tree_async as a plain model, shared by
tests/test_fold_edges_gpu.py (which judges the kernels by it) and
tests/test_fold_model.py (which checks it on the CPU first).

k = 2^L slots, bit q of `pres` set where slot q holds an operand (slot 0
always does).  Level m = 1, 2, 4, ...: slot s (bit m clear) = slot s OP
slot s + m, slot s the inout and slot s + m the in; where only one of the
two is present it passes through as a whole copy.  The result is slot 0."""
import numpy as np


def tree_steps(k, pres):
    """the fold as a list of steps over slot numbers, in order:
    ('op', s, s + m): slot s = slot s OP slot s + m (inout, in);
    ('copy', s, s + m): slot s, absent so far, takes slot s + m whole"""
    assert k >= 2 and k & (k - 1) == 0 and pres & 1 and pres < (1 << k)
    have = [bool((pres >> q) & 1) for q in range(k)]
    steps = []
    m = 1
    while m < k:
        for s in range(0, k, 2 * m):
            if have[s] and have[s + m]:
                steps.append(('op', s, s + m))
            elif have[s + m]:
                steps.append(('copy', s, s + m))
                have[s] = True
        m *= 2
    return steps


def tree_levels(vals, pres, f):
    """the level-by-level fold of the slot values `vals` under f(inout, in)"""
    v = list(vals)
    for kind, s, t in tree_steps(len(v), pres):
        v[s] = f(v[s], v[t]) if kind == 'op' else v[t]
    return v[0]


def tree_recursive(vals, pres, f):
    """the same fold as a recursion over slot ranges: the left half is the
    inout, the right half the in, an absent half passes the other through"""
    def fold(lo, n):
        if n == 1:
            return ((pres >> lo) & 1) == 1, vals[lo]
        ha, a = fold(lo, n // 2)
        hb, b = fold(lo + n // 2, n // 2)
        if ha and hb:
            return True, f(a, b)
        return ha or hb, (b if hb else a)
    have, r = fold(0, len(vals))
    assert have
    return r


def odd_upper_absent(k):
    """every odd slot above k/2 absent: what the fold of a non-power-of-two
    world leaves (the pattern of test_gpu_parity.test_tree_combine)"""
    absent = {q for q in range(k) if q % 2 and q > k // 2} if k >= 4 else set()
    return sum(1 << q for q in range(k) if q not in absent)


def masks_for(k):
    """the presence masks the suites run at k slots (slot 0 always present):
    every mask up to k = 8; at k = 16 only slot 0, all sixteen, the low w
    slots for w = 9..15, odd_upper_absent and 64 masks from a fixed seed"""
    if k <= 8:
        return [m for m in range(1 << k) if m & 1]
    assert k == 16
    rng = np.random.default_rng(0x5EED0F01)
    fixed = [1, 0xffff] + [(1 << w) - 1 for w in range(9, 16)] + [odd_upper_absent(16)]
    return fixed + [int(m) | 1 for m in rng.integers(0, 1 << 16, 64)]
