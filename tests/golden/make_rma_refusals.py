#!/usr/bin/env python3
"""Record what every RMA-style entry of libmpix_redop.so answers to a grid of
arguments that never reach a kernel: tests/golden/rma_refusals.json, replayed
by tests/test_rma_refusals.py.

CPU only.  Wild pointers stand for buffers (as in tests/test_getacc_cpu.py):
a call that is refused, or that has nothing to do, never looks at them, and
one that passes every argument check ends at the placement check with
MPI_ERR_BUFFER.  One abstract case -- operands, count, blocklen, stride, type,
op -- is handed to every entry of the families it names, each taking the
arguments it has; duplicate calls drop out.

The axes: count -1 / 0 / 1 / 16; blocklen and stride including stride <
blocklen and blocklen <= 0; a legal op, an illegal op, MPI_OP_NULL, MPIX_EQUAL,
MPI_NO_OP, MPI_REPLACE and a handle that is no op; covered types of 1-, 2-, 4-,
8-, 16- and 32-byte extent, a declined pair (MPIX_BFLOAT16 with MPI_MAX) and
an unknown type; each operand NULL and MPI_IN_PLACE (-1); each pair of
operands overlapping by one element, either way round; a target off its
extent's grid; an iov offset off that grid and an iovec length that is no
whole element; a NULL plan.

The file: "cases" lists [what the case changes in the replay's DEFAULTS, the
return codes of its calls in the order of the replay's calls()].

Run against the built library:  python tests/golden/make_rma_refusals.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from mpich_amd import handles as H                  # noqa: E402
from tests.test_rma_refusals import DEFAULTS, call_row, calls    # noqa: E402

O, R_, T, C = (DEFAULTS[k] for k in 'ortc')     # origin, result, target, compare
NOT_AN_OP = 0x12345678
UNKNOWN_TYPE = 0x4c0000ff

# (datatype, extent, a legal op, an illegal op): one of every extent first
TYPES = [
    (H.MPI_INT8_T, 1, H.MPI_SUM, H.MPI_MAXLOC),
    (H.MPI_SHORT, 2, H.MPI_BAND, H.MPI_MAXLOC),
    (H.MPI_FLOAT, 4, H.MPI_SUM, H.MPI_BAND),
    (H.MPI_DOUBLE, 8, H.MPI_SUM, H.MPI_BXOR),
    (H.MPI_DOUBLE_INT, 16, H.MPI_MINLOC, H.MPI_SUM),
    (H.MPI_LONG_DOUBLE_INT, 32, H.MPI_MAXLOC, H.MPI_SUM),
    (H.MPI_LONG, 8, H.MPI_MAX, H.MPI_MAXLOC),
    (H.MPI_INTEGER16, 16, H.MPI_SUM, H.MPI_MAXLOC),
    (H.MPIX_BFLOAT16, 2, H.MPI_MAX, H.MPI_BAND),        # legal, declined: no kernel
    (UNKNOWN_TYPE, 0, H.MPI_SUM, H.MPI_MAXLOC),
]
REAL = TYPES[:8]
ALL_OPS = [H.MPI_SUM, H.MPI_BAND, H.MPI_OP_NULL, H.MPIX_EQUAL, H.MPI_NO_OP, H.MPI_REPLACE,
           NOT_AN_OP]       # for MPI_FLOAT: legal, illegal, ...
ACC_OPS = [H.MPI_SUM, H.MPI_NO_OP, H.MPI_REPLACE]
COUNTS = [-1, 0, 1, 16]
SHAPES = [(2, 5), (4, 4), (3, 2), (0, 5), (-1, 2)]      # (blocklen, stride) beside (1, 1)


def case(fam, **over):
    """what a case changes in DEFAULTS; its type's extent goes with the type"""
    over = dict(over, fam=fam)
    if 'dt' in over:
        over['ext'] = next(e for d, e, _, _ in TYPES if d == over['dt']) or 4
    return {k: v for k, v in over.items() if DEFAULTS[k] != v}


def both_shapes(fam, **kw):
    """the contiguous entries take the case as it is, the others as a (2, 5) vector"""
    return [case(fam, **kw), case('vip', bl=2, st=5, **kw)]


def cases():
    out = []
    for dt, ext, legal, illegal in TYPES:           # type x op
        for op in (ALL_OPS[:6] if dt == H.MPI_FLOAT
                   else [legal, illegal, H.MPI_NO_OP, H.MPI_REPLACE]):
            out += both_shapes('c', dt=dt, op=op)
        out.append(case('s', dt=dt))
    for dt, ext, legal, _ in TYPES:                 # type x count
        for count in ((-1, 0, 1) if dt == H.MPI_FLOAT else (-1, 0)):
            out += both_shapes('c', dt=dt, op=legal, count=count)
    for count in COUNTS:                            # op x count x shape
        for op in ALL_OPS:
            out.append(case('c', op=op, count=count))
        for bl, st in SHAPES:
            for op in (H.MPI_SUM, H.MPI_REPLACE):
                out.append(case('v', op=op, count=count, bl=bl, st=st))
        for bl, st in SHAPES[:4]:
            out.append(case('ip', count=count, bl=bl, st=st))
    for dt, ext, legal, _ in (TYPES[0], TYPES[2], TYPES[5]):    # the caps on count * extent
        out.append(case('cv', dt=dt, op=legal, count=((1 << 56) // ext) + 1))
        out.append(case('v', dt=dt, op=legal, count=1 << 40, bl=1, st=1 << 20))
    for bad in (None, -1):                          # each operand NULL / MPI_IN_PLACE
        for which in 'ortc':
            for op in ACC_OPS:
                out += both_shapes('c', **{which: bad}, op=op)
            out += both_shapes('cs', **{which: bad}, count=0)
        out += both_shapes('cs', o=bad, r=bad, t=bad, c=bad)
    base = dict(o=O, r=R_, t=T, c=C)
    for dt, ext, legal, _ in (TYPES[2], TYPES[4], TYPES[0], TYPES[3], TYPES[5]):
        full = dt in (H.MPI_FLOAT, H.MPI_DOUBLE_INT)    # pairwise overlaps by one element
        for fam, bl, st in (('c', 1, 1), ('vip', 2, 5)):
            count = 16
            packed, span = count * bl * ext, ((count - 1) * st + bl) * ext
            size = dict(o=packed, r=packed, t=span)
            for x, y in ('ot', 'or', 'rt'):
                for a, b in ((x, y), (y, x)):       # b starts in a's last element
                    for op in (ACC_OPS[1:] + [legal] if full else [legal]):
                        out.append(case(fam, **{b: base[a] + size[a] - ext}, dt=dt, op=op,
                                        count=count, bl=bl, st=st))
            out.append(case(fam, o=O, r=O, t=O, c=O, dt=dt, op=legal, bl=bl, st=st))
    for dt, ext, legal, _ in REAL:
        # compare-and-swap looks at one element
        for x, y in ('ot', 'or', 'rt', 'oc', 'cr', 'ct'):
            out.append(case('s', **{y: base[x]}, dt=dt))
        out.append(case('cs', t=T + 1, dt=dt, op=legal))       # a target off its extent's grid
        out.append(case('c', t=T + 1, dt=dt, op=H.MPI_REPLACE))
        out.append(case('c', t=T + 1, dt=dt, op=legal, count=0))
        out.append(case('cs', t=T + ext // 2, dt=dt, op=legal))
    out.append(case('v', t=T + 1, bl=2, st=5))
    for dt, ext, legal, _ in (TYPES[1], TYPES[3], TYPES[4]):    # iov tables off the grid
        for kind in ('offset', 'length'):
            for op in (legal, H.MPI_NO_OP):
                out.append(case('ip', dt=dt, op=op, bl=2, st=5, iov=kind))
        out.append(case('ip', dt=dt, op=legal, count=0, bl=2, st=5, iov='offset'))
        out.append(case('ip', dt=dt, op=legal, iov='null'))
        out.append(case('ip', dt=dt, op=legal, iov='negative'))
    for op in ALL_OPS:                              # a NULL plan
        out.append(case('p', op=op, plan=False))
        out.append(case('p', op=op, plan=False, o=None, r=None, t=None))
    return out


def main():
    seen, out, classes = set(), [], {}
    for over in cases():
        codes = []
        for func, args in calls(dict(DEFAULTS, **over)):
            rc, err = call_row(func, args)
            assert rc == err, (func, args, rc, err)
            codes.append(rc)
            key = json.dumps([func, args])
            if key not in seen:
                seen.add(key)
                classes.setdefault(func, {}).setdefault(rc, 0)
                classes[func][rc] += 1
        out.append(json.dumps([over, codes], separators=(',', ':')))
    for func in sorted(classes):
        print('%-46s %s' % (func, sorted(classes[func].items())))
    print(len(out), 'cases,', len(seen), 'distinct calls')
    with open(os.path.join(HERE, 'rma_refusals.json'), 'w') as f:
        f.write('{"cases": [\n%s\n]}\n' % ',\n'.join(out))


if __name__ == '__main__':
    main()
