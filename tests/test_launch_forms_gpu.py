"""Every kernel form the launch plans name (mpich_amd/csrc/redop_launch.h),
run once on the GPU through the public entry that takes it.

The cases are those of tests/golden/launch_plans.json: for every entry
(contiguous, multi, tree, vector, get-accumulate) and every form it can take
one test, which runs, for every unit size below, the fixture case with the
fewest elements this test can run -- a packet form's
with at least one packet before one without: a head, one packet and a tail, or
one 64-packet tile and a packet, at the fixture's phases, a few KiB at the
most -- and per unit width the smallest batch that holds a call of its own, a
table slot and a launch.  A case runs with the types fp32 SUM (4-byte unit),
int8 MAX (1), DOUBLE_INT MAXLOC (16), LONG_DOUBLE_INT MAXLOC and
C_LONG_DOUBLE_COMPLEX PROD (32, the second a split combiner; a case that names
`is_split` takes the one it names), the operands placed at the case's 16-byte
phases under its launch settings (block, max_grid), operands the fixture gives
one address sharing a buffer.  The result equals the oracle's bit for bit over
the type map, every input is unchanged and the guard bytes on both sides of
every operand are intact.  A form of the enum without a case here fails
test_every_form_has_a_case.

Not run here (tests/test_launch_plan.py replays them on the CPU): the batch's
flush before a segment that would pass max_blocks and its segment with more
tiles than one grid holds -- both need 2^26 blocks, tens of GiB; the fixture's
2- and 8-byte units, whose forms the units above take too; tree cases with
k = 3, 5, 9 or slot 0 absent, which the public entry refuses."""
import json
import os

import numpy as np
import pytest
import torch

from tests import fold_model as M
from tests.test_getacc_gpu import CANARY, Placed, _soft_operands, field_mask
from tests.test_launch_plan import forms_of_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 1 << 12      # make_launch_plans.py: operand slot q at q * BASE + phase
MAX_BYTES = 32 << 10
TYPES = {1: [('MPI_INT8_T', 'MPI_MAX')], 4: [('MPI_FLOAT', 'MPI_SUM')],
         16: [('MPI_DOUBLE_INT', 'MPI_MAXLOC')],
         32: [('MPI_LONG_DOUBLE_INT', 'MPI_MAXLOC'), ('MPI_C_LONG_DOUBLE_COMPLEX', 'MPI_PROD')]}
PACKET_FORMS = {'PacketsAin', 'PacketsUin', 'Tree2x2', 'Tree4x2', 'Tree8x1', 'Tree16x1',
                'GetaccAligned', 'GetaccUnaligned'}

with open(os.path.join(ROOT, 'tests', 'golden', 'launch_plans.json')) as _f:
    GOLD = json.load(_f)['cases']


def shape(c):
    """(elements of the largest operand, block, max_grid, is_split or None) of a case"""
    kind = c[0]
    if kind == 'contig':
        return c[4], c[5], c[6], None
    if kind == 'multi':
        return c[4], c[5], c[6], None
    if kind == 'tree':
        return c[4], 256, c[5], c[6] if c[1] == 32 else None
    if kind == 'vector':
        n, bl, st = c[4:7]
        return (n // bl - 1) * st + bl, c[7], c[8], None
    if kind == 'getacc':
        return c[5], c[6], c[7], None
    return max(s[2] for s in c[2]), c[3], 0, c[4] if c[1] == 32 else None


def runnable(c):
    kind, unit = c[0], c[1]
    if unit not in TYPES or not 1 <= shape(c)[0] * unit <= MAX_BYTES:
        return False
    if kind == 'contig':
        return c[7] == 0 and c[8] == 0      # the completion word is the synchronous entry's
    if kind == 'tree':
        k = len(c[2])
        return k in (2, 4, 8, 16) and c[2][0] != 0
    return True


def picks():
    best = {}
    for c in GOLD:
        if not runnable(c):
            continue
        if c[0] == 'batch':
            if {s[0] for s in c[-1]} < ({'O'} if c[4] else {'O', 'S', 'F'}):
                continue
            key, rank = ('batch', c[1], c[4]), sum(s[2] for s in c[2])
        else:
            form = c[-10]
            key = (c[0], form, c[1])
            rank = (form in PACKET_FORMS and c[-3] == 0, shape(c)[0])
        if key not in best or rank < best[key][0]:
            best[key] = (rank, c)
    return [best[k][1] for k in sorted(best, key=str)]


PICKS = picks()


def groups():
    """the picks of one entry and form over every unit size (a batch: of every
    unit width and combiner kind), one test each"""
    out = {}
    for c in PICKS:
        out.setdefault(c[0] if c[0] == 'batch' else '%s-%s' % (c[0], c[-10]), []).append(c)
    return out


GROUPS = groups()


def case_id(c):
    return '-'.join(str(x) for x in ((c[0], c[1], 'split' if c[4] else 'plain') if c[0] == 'batch'
                                     else (c[0], c[-10], c[1])))


def test_every_form_has_a_case():
    ran = {c[-10] for c in PICKS if c[0] != 'batch'}
    assert ran == forms_of_header(), forms_of_header() - ran
    # and a batch of either unit width, and a split combiner's
    assert {(c[1] > 16, c[4]) for c in PICKS if c[0] == 'batch'} >= {(False, 0), (True, 0), (True, 1)}


@pytest.fixture(scope='module')
def R():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from mpich_amd import redop
    assert redop.lib().MPIX_Redop_init() == 0
    return redop


@pytest.fixture(scope='module')
def H():
    from mpich_amd import handles
    return handles


@pytest.fixture(scope='module')
def operands(H):
    """eighteen operands of MAX_BYTES per type, made once: (n, ext) bytes"""
    rng = np.random.default_rng(0x5EED0A11)
    out = {}
    n = MAX_BYTES // 4
    out['MPI_FLOAT'] = [rng.uniform(-1, 1, n).astype('<f4').view(np.uint8).reshape(n, 4)
                        for _ in range(18)]
    n = MAX_BYTES // 16
    out['MPI_INT8_T'] = [rng.integers(0, 256, (MAX_BYTES, 1), dtype=np.uint8) for _ in range(18)]
    pairs = []
    for _ in range(18):     # values from a small range: ties; random padding
        p = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        p[:, :8] = rng.integers(0, 16, n).astype('<f8').view(np.uint8).reshape(n, 8)
        p[:, 8:12] = rng.integers(-3, 4, n).astype('<i4').view(np.uint8).reshape(n, 4)
        pairs.append(p)
    out['MPI_DOUBLE_INT'] = pairs
    for dtname in ('MPI_LONG_DOUBLE_INT', 'MPI_C_LONG_DOUBLE_COMPLEX'):
        xs = []
        for _ in range(9):
            xs += [np.ascontiguousarray(x).view(np.uint8).reshape(-1, 32)
                   for x in _soft_operands(H, rng, dtname, MAX_BYTES // 32, False)]
        out[dtname] = xs
    return out


class Bufs:
    """the operands of one call: fixture address -> a Placed buffer of `n`
    elements at the address's phase, one buffer per address slot"""

    def __init__(self, data, ext):
        self.data, self.ext, self.slots = data, ext, {}

    def at(self, addr, n, fill=None):
        slot = addr // BASE
        if slot not in self.slots:
            src = self.data[len(self.slots)][:n] if fill is None else np.full((n, self.ext), fill,
                                                                             np.uint8)
            assert len(src) == n
            host = np.ascontiguousarray(src).reshape(-1).copy()
            self.slots[slot] = (Placed(host, addr % BASE), host)
        p, host = self.slots[slot]
        assert (p.v.data_ptr() - addr) % 64 == 0 and p.nb == n * self.ext
        return p, host

    def check_inputs_and_guards(self, outputs, ctx):
        for p, host in self.slots.values():
            assert p.guards_intact(), ('guard bytes', ctx)
            if not any(p is o for o in outputs):
                assert np.array_equal(p.bytes(), host), ('input changed', ctx)


def same(got, exp, fields, ext, ctx):
    got, exp = got.reshape(-1, ext)[:, fields], exp.reshape(-1, ext)[:, fields]
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, (ctx, 'elements', bad[:8].tolist(), len(bad))


def run_case(R, H, oracle, operands, case):
    kind, unit = case[0], case[1]
    _, block, max_grid, is_split = shape(case)
    types = TYPES[unit] if is_split is None else [TYPES[unit][is_split]]
    prev = R.get_launch()
    assert R.set_launch(block, max_grid) == 0
    try:
        for dtname, opname in types:
            dt, op = getattr(H, dtname), getattr(H, opname)
            ext = R.datatype_extent(dt)
            assert ext == unit
            fields = field_mask(H, dt, ext)
            B = Bufs(operands[dtname], ext)
            ctx = (case_id(case), dtname, opname)

            def fold(inout, inb, n):
                exp = inout.copy()
                assert oracle.reduce_local(inb.copy(), exp, n, dt, op) == 0
                return exp
            torch.cuda.synchronize()
            if kind == 'contig':
                ai, ao, n = case[2:5]
                (I, hi), (O, ho) = B.at(ai, n), B.at(ao, n)
                assert R.reduce_local_async(I.v, O.v, n, dt, op) == 0, ctx
                same(O.bytes(), fold(ho, hi, n), fields, ext, ctx)
                outs = [O]
            elif kind == 'multi':
                ins, ao, n = case[2:5]
                O, ho = B.at(ao, n)
                Is = [B.at(a, n) for a in ins]
                assert R.reduce_local_multi_async([p.v for p, _ in Is], O.v, n, dt, op) == 0, ctx
                exp = ho
                for _, h in Is:
                    exp = fold(exp, h, n)
                same(O.bytes(), exp, fields, ext, ctx)
                outs = [O]
            elif kind == 'tree':
                ins, ao, n = case[2:5]
                Is = [B.at(a, n) if a else None for a in ins]
                O, _ = B.at(ao, n, fill=CANARY)
                pres = sum(1 << q for q, a in enumerate(ins) if a)
                exp = M.tree_levels([None if x is None else x[1] for x in Is], pres,
                                    lambda a, b: fold(a, b, n))
                assert R.reduce_local_tree_async([None if x is None else x[0].v for x in Is], O.v,
                                                 n, dt, op) == 0, ctx
                same(O.bytes(), exp, fields, ext, ctx)
                outs = [O]
            elif kind == 'vector':
                ai, ao, n, bl, st = case[2:7]
                count = n // bl
                span = (count - 1) * st + bl
                (I, hi), (O, ho) = B.at(ai, n), B.at(ao, span)
                assert R.reduce_local_vector(I.v, O.v, count, bl, st, dt, op) == 0, ctx
                idx = (np.arange(count)[:, None] * st + np.arange(bl)[None, :]).reshape(-1)
                exp = ho.reshape(span, ext).copy()
                exp[idx] = fold(np.ascontiguousarray(exp[idx]).reshape(-1), hi, n).reshape(n, ext)
                got = O.bytes().reshape(span, ext)
                same(got[idx], exp[idx], fields, ext, ctx)
                gaps = np.setdiff1d(np.arange(span), idx)
                assert np.array_equal(got[gaps], exp[gaps]), ('gap elements', ctx)
                outs = [O]
            elif kind == 'getacc':
                ai, ar, ao, n = case[2:6]
                (I, hi), (O, ho) = B.at(ai, n), B.at(ao, n)
                Z, _ = B.at(ar, n, fill=CANARY)
                assert R.get_accumulate_local(I.v, Z.v, O.v, n, dt, op) == 0, ctx
                same(O.bytes(), fold(ho, hi, n), fields, ext, ctx)
                res = Z.bytes().reshape(n, ext)
                same(res, ho, fields, ext, ctx + ('result',))
                assert (res[:, ~fields] == CANARY).all(), ('result padding', ctx)
                outs = [O, Z]
            else:
                segs = case[2]
                Is = [B.at(s[0], s[2]) if s[2] else None for s in segs]
                Os = [B.at(s[1], s[2]) if s[2] else None for s in segs]
                none = torch.zeros(2 * len(segs), 64, dtype=torch.uint8, device='cuda')
                assert R.reduce_local_batch_async(
                    [none[2 * i] if x is None else x[0].v for i, x in enumerate(Is)],
                    [none[2 * i + 1] if x is None else x[0].v for i, x in enumerate(Os)],
                    [s[2] for s in segs], dt, op) == 0, ctx
                for s, i, o in zip(segs, Is, Os):
                    if s[2]:
                        same(o[0].bytes(), fold(o[1], i[1], s[2]), fields, ext, ctx + (s,))
                outs = [o[0] for o in Os if o]
            B.check_inputs_and_guards(outs, ctx)
    finally:
        R.set_launch(prev['block'], prev['max_grid'])


@pytest.mark.gpu
@pytest.mark.parametrize('group', sorted(GROUPS))
def test_form(R, H, oracle, operands, group):
    for case in GROUPS[group]:
        run_case(R, H, oracle, operands, case)
