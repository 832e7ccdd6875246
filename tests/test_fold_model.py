"""tests/fold_model.py, the reference the fold suite on the GPU judges the tree
kernels by, against an independent formulation on the CPU: the level-by-level
fold (tree_fold in redop_kernels.h) and the recursion over slot ranges
(tree_fold_rec) must agree for every presence mask the GPU suite runs, under
a function that is neither commutative nor associative."""
import pytest

from tests import fold_model as M


def paren(a, b):
    return '(%s.%s)' % (a, b)


@pytest.mark.parametrize('k', [2, 4, 8, 16])
def test_levels_equal_the_recursion(k):
    vals = ['s%d' % q for q in range(k)]
    masks = M.masks_for(k)
    assert all(m & 1 and m < (1 << k) for m in masks)
    if k <= 8:
        assert len(masks) == 1 << (k - 1) and len(set(masks)) == len(masks)
    else:
        assert len(masks) == 74 and {1, 0xffff, 0x1ff, 0x7fff, M.odd_upper_absent(16)} <= set(masks)
    for pres in masks:
        got = M.tree_levels(vals, pres, paren)
        assert got == M.tree_recursive(vals, pres, paren), bin(pres)
        # every present slot exactly once and in slot order, no absent one
        flat = got.replace('(', '').replace(')', '').split('.')
        assert flat == [vals[q] for q in range(k) if (pres >> q) & 1], bin(pres)


def test_known_shapes():
    v = list('abcdefgh')
    assert M.tree_levels(v[:2], 0b11, paren) == '(a.b)'
    assert M.tree_levels(v[:2], 0b01, paren) == 'a'
    assert M.tree_levels(v[:4], 0b1111, paren) == '((a.b).(c.d))'
    assert M.tree_levels(v[:4], 0b1001, paren) == '(a.d)'
    assert M.tree_levels(v[:4], 0b1101, paren) == '(a.(c.d))'
    assert M.tree_levels(v, 0xff, paren) == '(((a.b).(c.d)).((e.f).(g.h)))'
    assert M.tree_levels(v, 0b10100101, paren) == '((a.c).(f.h))'
    assert M.tree_levels(v, M.odd_upper_absent(8), paren) == '(((a.b).(c.d)).(e.g))'


@pytest.mark.parametrize('k', [2, 4, 8, 16])
def test_replace_and_no_op(k):
    """MPI_REPLACE (inout = in) folds to the last present slot, MPI_NO_OP
    (inout kept) to the first: what the entry resolves on the host"""
    vals = list(range(k))
    for pres in M.masks_for(k):
        last = max(q for q in range(k) if (pres >> q) & 1)
        for fold in (M.tree_levels, M.tree_recursive):
            assert fold(vals, pres, lambda a, b: b) == last
            assert fold(vals, pres, lambda a, b: a) == 0


def test_steps_touch_present_slots_only():
    for k in (2, 4, 8, 16):
        for pres in M.masks_for(k):
            have = {q for q in range(k) if (pres >> q) & 1}
            for kind, s, t in M.tree_steps(k, pres):
                assert t in have and t > s
                assert (s in have) == (kind == 'op')
                have.add(s)
