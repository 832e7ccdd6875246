"""Replay of the recorded refusal table of the RMA-style entries
(tests/golden/rma_refusals.json, written by tests/golden/make_rma_refusals.py
from the library as it stood before their host-side scaffolding was shared).

The file holds abstract cases and, for each, the return code of every call
made from it (calls() below); a row is one such (C function, arguments, code).
Wild pointers stand for buffers, so a row ends at a refusal, at "nothing to
do", or at the placement check -- on a machine with or without a GPU.  The
replay asserts the same code for every row and that MPIX_Redop_last_error()
agrees; the order of the checks is public behaviour (include/mpix_redop.h
numbers them), and this table pins it for every entry at once."""
import ctypes
import json
import os

import pytest

from mpich_amd import handles as H
from mpich_amd import redop as R

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rma_refusals.json')

OK, BUF, CNT, TYP, OP, ARG = (H.MPI_SUCCESS, H.MPI_ERR_BUFFER, H.MPI_ERR_COUNT, H.MPI_ERR_TYPE,
                              H.MPI_ERR_OP, H.MPI_ERR_ARG)

# Every entry in the table's scope and the classes it can return before any
# device is needed (read off the numbered checks in include/mpix_redop.h).
# The synchronous reduce-vector entry classifies its target first, so wild
# pointers only ever get MPI_ERR_BUFFER from it; compare-and-swap takes no
# count and no op; a plan's counts were checked when it was created.
CLASSES = {
    'MPIX_Get_accumulate_local': {OK, BUF, CNT, TYP, OP},
    'MPIX_Get_accumulate_local_async': {OK, BUF, CNT, TYP, OP},
    'MPIX_Get_accumulate_local_vector': {OK, BUF, CNT, TYP, OP, ARG},
    'MPIX_Get_accumulate_local_vector_async': {OK, BUF, CNT, TYP, OP, ARG},
    'MPIX_Get_accumulate_local_iov_async': {OK, BUF, CNT, TYP, OP, ARG},
    'MPIX_Get_accumulate_local_iovec_async': {OK, BUF, CNT, TYP, OP, ARG},
    'MPIX_Get_accumulate_local_plan': {OK, BUF, TYP, OP, ARG},
    'MPIX_Get_accumulate_local_plan_async': {OK, BUF, TYP, OP, ARG},
    'MPIX_Reduce_local_vector': {BUF},
    'MPIX_Reduce_local_vector_async': {OK, BUF, CNT, TYP, OP, ARG},
    'MPIX_Reduce_local_iov_async': {OK, BUF, CNT, TYP, OP},
    'MPIX_Reduce_local_iovec_async': {OK, BUF, CNT, TYP, OP, ARG},
    'MPIX_Reduce_local_plan': {OK, BUF, TYP, OP, ARG},
    'MPIX_Reduce_local_plan_async': {OK, BUF, TYP, OP, ARG},
    'MPIX_Compare_and_swap_local': {BUF, TYP},
    'MPIX_Compare_and_swap_local_async': {BUF, TYP},
    'MPIX_Accumulate_local_atomic': {OK, BUF, CNT, TYP, OP},
    'MPIX_Accumulate_local_atomic_async': {OK, BUF, CNT, TYP, OP},
    'MPIX_Get_accumulate_local_atomic': {OK, BUF, CNT, TYP, OP},
    'MPIX_Get_accumulate_local_atomic_async': {OK, BUF, CNT, TYP, OP},
    'MPIX_Compare_and_swap_local_atomic': {BUF, TYP},
    'MPIX_Compare_and_swap_local_atomic_async': {BUF, TYP},
}


def call_row(func, args):
    """One row's call.  A list argument is an MPIX_Aint array, a dict a plan
    to create from {nseg, offs, counts, dt} (NULL if the create refuses it);
    an _async entry gets the null stream.  Returns (rc, last_error)."""
    L = R.lib()
    aint = ctypes.c_ssize_t
    plans, cargs = [], []
    for a in args:
        if isinstance(a, dict):
            p = ctypes.c_void_p()
            offs = (aint * max(len(a['offs']), 1))(*a['offs'])
            cnts = (aint * max(len(a['counts']), 1))(*a['counts'])
            L.MPIX_Iov_plan_create(a['nseg'], offs, cnts, H.as_c_int(a['dt']), ctypes.byref(p))
            plans.append(p)
            cargs.append(p.value)
        elif isinstance(a, list):
            cargs.append((aint * max(len(a), 1))(*a))
        else:
            cargs.append(a)
    if func.endswith('_async'):
        cargs.append(None)
    f = getattr(L, func)
    cargs = [H.as_c_int(a) if t is ctypes.c_int else a for a, t in zip(cargs, f.argtypes)]
    rc = f(*cargs)
    err = L.MPIX_Redop_last_error()
    for p in plans:
        L.MPIX_Iov_plan_free(ctypes.byref(p))
    return rc, err


# One abstract case -- operands, count, blocklen, stride, type, op -- is handed
# to every entry of the families it names, each taking the arguments it has.
# fam: c contiguous (get-accumulate and the atomic forms), s both
# compare-and-swaps, v vector, i iov / iovec, p plan.  iov: what is wrong with
# the table ('offset', 'length', 'negative', 'null'); plan False: a NULL plan.
DEFAULTS = dict(fam='c', o=0x100000, r=0x200000, t=0x300000, c=0x400000, count=16, bl=1, st=1,
                dt=H.MPI_FLOAT, ext=4, op=H.MPI_SUM, iov=None, plan=True)


def table(k):
    """the case's vector as an iov table: (nseg, byte offsets, element counts)"""
    n, ext = k['count'], k['ext']
    if n < 0:
        return n, [], []
    offs = [i * k['st'] * ext for i in range(n)]
    cnts = [k['bl']] * n
    if k['iov'] == 'offset' and n:
        offs[-1] += 1
        if ext > 4:
            offs[0] += 2
    if k['iov'] == 'negative' and n:
        cnts[-1] = -1
    return n, offs, cnts


def calls(k):
    """the case's calls, in the order of its recorded codes: (C function, arguments)"""
    o, r, t, c, dt, op = k['o'], k['r'], k['t'], k['c'], k['dt'], k['op']
    count, bl, st, fam = k['count'], k['bl'], k['st'], k['fam']
    out = []

    def both(entry, args):
        out.extend([(entry, args), (entry + '_async', args)])
    if 'c' in fam:
        both('MPIX_Get_accumulate_local', [o, r, t, count, dt, op])
        both('MPIX_Accumulate_local_atomic', [o, t, count, dt, op])
        both('MPIX_Get_accumulate_local_atomic', [o, r, t, count, dt, op])
    if 's' in fam:
        both('MPIX_Compare_and_swap_local', [o, c, r, t, dt])
        both('MPIX_Compare_and_swap_local_atomic', [o, c, r, t, dt])
    if 'v' in fam:
        both('MPIX_Get_accumulate_local_vector', [o, r, t, count, bl, st, dt, op])
        both('MPIX_Reduce_local_vector', [o, t, count, bl, st, dt, op])
    if not ('i' in fam or 'p' in fam):
        return out
    nseg, offs, cnts = table(k)
    if k['iov'] == 'null':
        offs, cnts = None, None
    lens = None if cnts is None else [n * k['ext'] for n in cnts]
    if k['iov'] == 'length' and lens:
        lens[-1] += 1
    if 'i' in fam:
        for form, tab in (('iov', cnts), ('iovec', lens)):
            out.append(('MPIX_Get_accumulate_local_%s_async' % form,
                        [o, r, t, nseg, offs, tab, dt, op]))
            out.append(('MPIX_Reduce_local_%s_async' % form, [o, t, nseg, offs, tab, dt, op]))
    if 'p' in fam and k['iov'] != 'length':
        plan = None
        if k['plan'] and offs is not None and nseg >= 0:
            plan = dict(nseg=nseg, offs=offs, counts=cnts, dt=dt)
        both('MPIX_Get_accumulate_local_plan', [o, r, t, plan, op])
        both('MPIX_Reduce_local_plan', [o, t, plan, op])
    return out


@pytest.fixture(scope='module')
def rows():
    """the file's cases ([what differs from DEFAULTS, the codes of calls(case)])
    as (C function, arguments, code)"""
    with open(TABLE) as f:
        doc = json.load(f)
    out = []
    for over, codes in doc['cases']:
        todo = calls(dict(DEFAULTS, **over))
        assert len(todo) == len(codes), over
        out += [(func, args, rc) for (func, args), rc in zip(todo, codes)]
    return out


def test_every_row_replays(rows):
    bad = []
    for func, args, want in rows:
        rc, err = call_row(func, args)
        if rc != want or err != want:
            bad.append((func, args, want, rc, err))
    assert not bad, '%d of %d rows differ, first: %r' % (len(bad), len(rows), bad[:5])


def test_table_covers_every_entry_and_class(rows):
    """a thinned-out table fails: every entry in scope is there with at least
    one row of each class it can return without a device, and no other"""
    seen = {}
    for func, _, want in rows:
        seen.setdefault(func, set()).add(want)
    assert set(seen) == set(CLASSES)
    for func, classes in CLASSES.items():
        assert seen[func] == classes, (func, sorted(seen[func]), sorted(classes))
    assert len(rows) >= 2000
