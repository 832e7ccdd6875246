"""Committed iov plans (MPIX_Iov_plan_*, MPIX_Reduce_local_plan*,
MPIX_Get_accumulate_local_plan*) on a machine without a GPU: every create
error class in its order, what _info reports about merging and grouping, the
launch entries' checks on wild pointers, that create / _info / _free make no
HIP call, what the new instantiation units hold, and the Python mirror's range
checks.

Wild pointers stand for buffers: a call that is refused, or that has nothing
to do, never looks at them."""
import ctypes
import os

import numpy as np
import pytest

from mpich_amd import handles as H
from mpich_amd import redop as R
from tests.test_getacc_iov_cpu import A, AINT, B, C, WILD, tab
from tests.test_kernel_resources import BUILD, OBJDUMP, READELF, _kernels
from tests.test_no_hip_init import _probe, shim  # noqa: F401  (shim is a fixture)

INT_MAX = 2 ** 31 - 1
TOP = 1 << 56


def create(offs, second, dt=H.MPI_DOUBLE, nseg=None, iovec=False, out=True):
    """(rc, handle): the handle must be NULL exactly when rc is an error"""
    f = R.lib().MPIX_Iov_plan_create_iovec if iovec else R.lib().MPIX_Iov_plan_create
    h = ctypes.c_void_p(0xdead)
    rc = f(len(offs) if nseg is None else nseg, None if offs is None else tab(offs),
           None if second is None else tab(second), H.as_c_int(dt),
           ctypes.byref(h) if out else None)
    assert R.lib().MPIX_Redop_last_error() == rc
    if out:
        assert (h.value is None) == (rc != 0), (rc, h.value)
    return rc, h


def err(*a, **k):
    rc, h = create(*a, **k)
    if rc == 0:
        assert R.lib().MPIX_Iov_plan_free(ctypes.byref(h)) == 0 and h.value is None
    return rc


def info(offs, second, dt=H.MPI_DOUBLE, iovec=False):
    with (R.IovPlan.from_iovec if iovec else R.IovPlan.from_iov)(offs, second, dt) as p:
        return p.info()


# ------------------------------------------------------------------- create
def test_create_errors_in_their_order():
    # nseg < 0, nseg > INT_MAX: before the tables, the type and the plan pointer
    for iovec in (False, True):
        assert err([0], [8], nseg=-1, iovec=iovec) == H.MPI_ERR_COUNT
        assert err(None, None, 0x4c0000ff, nseg=-1, iovec=iovec, out=False) == H.MPI_ERR_COUNT
        assert err(None, None, 0x4c0000ff, nseg=INT_MAX + 1, iovec=iovec) == H.MPI_ERR_COUNT
        # NULL tables
        assert err(None, [8], nseg=1, iovec=iovec) == H.MPI_ERR_BUFFER
        assert err([0], None, nseg=1, iovec=iovec) == H.MPI_ERR_BUFFER
        assert err(None, None, nseg=INT_MAX, iovec=iovec) == H.MPI_ERR_BUFFER   # INT_MAX itself passes
    # a negative count before the type (iov) ...
    assert err([0, 64], [2, -1]) == H.MPI_ERR_COUNT
    assert err([0], [-1], 0x4c0000ff) == H.MPI_ERR_COUNT
    # ... the iovec form looks up the type first
    assert err([0, 64], [16, -8], iovec=True) == H.MPI_ERR_COUNT
    assert err([0], [-8], 0x4c0000ff, iovec=True) == H.MPI_ERR_TYPE
    # a partial element (iovec) before the residue
    assert err([0], [12], iovec=True) == H.MPI_ERR_ARG
    assert err([2, 64], [16, 4], iovec=True) == H.MPI_ERR_ARG
    assert err([0, 4], [4, 4], H.MPI_FLOAT_INT, iovec=True) == H.MPI_ERR_ARG
    # an unknown type before the residue and the caps
    assert err([2], [1], 0x4c0000ff) == H.MPI_ERR_TYPE
    assert err([2], [TOP], 0x4c0000ff) == H.MPI_ERR_TYPE
    # a misaligned residue before the caps
    assert err([0, 66], [2, 2]) == H.MPI_ERR_ARG
    assert err([-10], [2]) == H.MPI_ERR_ARG
    assert err([1], [2], H.MPI_INT16_T) == H.MPI_ERR_ARG
    assert err([2], [TOP // 8]) == H.MPI_ERR_ARG
    assert err([0, 3], [4, 0]) == H.MPI_ERR_ARG     # a run that covers nothing counts, as in the entries
    assert err([3], [0]) == 0                       # ... unless the whole table covers nothing
    assert err([0, 68], [2, 2]) == 0                # 4 mod 8 is fine
    assert err([2], [2], H.MPI_INT16_T) == 0
    assert err([3], [2], H.MPI_INT8_T) == 0
    # the caps: packed range, the sum, the bounding range
    assert err([0], [TOP // 8]) == H.MPI_ERR_COUNT
    assert err([0], [TOP // 8 - 1]) == 0
    assert err([0, 0], [TOP // 16, TOP // 16]) == H.MPI_ERR_COUNT
    assert err([0, TOP - 8], [1, 1]) == H.MPI_ERR_COUNT
    assert err([0, TOP - 16], [1, 1]) == 0
    assert err([-(TOP // 2), TOP // 2 - 8], [1, 1]) == H.MPI_ERR_COUNT
    assert err([-(1 << 62), 1 << 62], [1, 1]) == H.MPI_ERR_COUNT
    assert err([0, 1 << 62], [1, 0]) == 0           # an empty run bounds nothing
    assert err([0], [TOP], iovec=True) == H.MPI_ERR_COUNT
    assert err([0], [(1 << 63) - 1]) == H.MPI_ERR_COUNT
    # a NULL plan pointer last
    assert err([0], [TOP // 8], out=False) == H.MPI_ERR_COUNT
    assert err([0], [4], out=False) == H.MPI_ERR_ARG
    assert err([], [], out=False) == H.MPI_ERR_ARG


def test_free_and_info_of_null():
    h = ctypes.c_void_p()
    assert R.lib().MPIX_Iov_plan_free(ctypes.byref(h)) == 0
    assert R.lib().MPIX_Iov_plan_free(None) == H.MPI_ERR_ARG
    assert R.lib().MPIX_Iov_plan_info(None, *[None] * 6) == H.MPI_ERR_ARG
    assert R.lib().MPIX_Iov_plan_prepare(None, 0) == H.MPI_ERR_ARG
    rc, h = create([0, 80], [4, 4])
    assert rc == 0 and R.lib().MPIX_Iov_plan_info(h, *[None] * 6) == 0      # every out pointer optional
    assert R.lib().MPIX_Iov_plan_free(ctypes.byref(h)) == 0 and h.value is None


# -------------------------------------------------------------------- _info
def test_info_empty_plans():
    empty = dict(elements=0, runs=0, groups=0, lo_byte=0, hi_byte=0, table_bytes=0)
    assert info([], []) == empty
    assert info([0, 64, -8], [0, 0, 0]) == empty
    # a padded pair's segment that never completes an element
    assert info([0], [8], H.MPI_DOUBLE_INT, iovec=True) == empty


def test_info_merging():
    # adjacent in call order: one run, no table
    assert info([0, 32, 64], [4, 4, 2]) == dict(elements=10, runs=1, groups=1, lo_byte=0,
                                                hi_byte=80, table_bytes=0)
    # adjacent in memory, out of call order: they stay apart
    i = info([32, 0], [4, 4])
    assert (i['elements'], i['runs'], i['groups'], i['lo_byte'], i['hi_byte']) == (8, 2, 1, 0, 64)
    # [seg_off 2][prefix 3][src_off 2] as 64-bit words, 1 tile + the closing entry as 32-bit
    assert i['table_bytes'] == 7 * 8 + 2 * 4
    # a zero-length run between two mergeable runs does not keep them apart
    assert info([0, 4096, 32], [4, 0, 4])['runs'] == 1
    assert info([0, 32, 32], [4, 0, 4])['runs'] == 1
    # a gap does
    assert info([0, 40], [4, 4])['runs'] == 2
    # a chain with one break
    i = info([8 * k for k in range(100)] + [808 + 8 * k for k in range(50)], [1] * 150)
    assert (i['elements'], i['runs'], i['lo_byte'], i['hi_byte']) == (150, 2, 0, 1208)
    # an overlapping restart is not adjacency
    assert info([0, 24], [4, 4])['runs'] == 2


def test_info_grouping_and_bounds():
    i = info([0, 84, 160, 244], [4, 4, 4, 4])           # residues 0, 4, 0, 4
    assert (i['runs'], i['groups']) == (4, 2)
    # two groups of two runs, 8 elements each
    assert i['table_bytes'] == 2 * (7 * 8 + 2 * 4)
    i = info([96, -64], [4, 4])
    assert (i['lo_byte'], i['hi_byte'], i['runs'], i['groups']) == (-64, 128, 2, 1)
    i = info([-12, -100], [1, 2])                       # residue 4, both below the pointer
    assert (i['lo_byte'], i['hi_byte'], i['groups']) == (-100, -4, 1)
    i = info([-24], [3])
    assert (i['lo_byte'], i['hi_byte'], i['runs'], i['table_bytes']) == (-24, 0, 1, 0)
    # the tile index grows with the packed elements: 700 elements in two runs, 3 tiles + 1
    assert info([0, 8000], [300, 400])['table_bytes'] == 7 * 8 + 4 * 4


def test_info_double_int_raw_iovec_is_one_run():
    """37 contiguous MPI_DOUBLE_INT elements as their raw iov: {double, int}
    per element, 74 segments; gathered into 37 runs of one element at extent
    stride, which merge into one"""
    offs, lens = [], []
    for k in range(37):
        offs += [16 * k, 16 * k + 8]
        lens += [8, 4]
    assert len(offs) == 74
    assert info(offs, lens, H.MPI_DOUBLE_INT, iovec=True) == dict(
        elements=37, runs=1, groups=1, lo_byte=0, hi_byte=37 * 16, table_bytes=0)


# ------------------------------------------------------- the launch entries
def plan_of(offs, cnts, dt=H.MPI_DOUBLE):
    rc, h = create(offs, cnts, dt)
    assert rc == 0
    return h


def launches(h, origin, result, target, op=H.MPI_SUM):
    """(reduce async, reduce sync, fetch async, fetch sync) error classes; the
    reduce forms take origin as their source"""
    L = R.lib()
    out = []
    for f, args in ((L.MPIX_Reduce_local_plan_async, (origin, target, h, H.as_c_int(op), None)),
                    (L.MPIX_Reduce_local_plan, (origin, target, h, H.as_c_int(op))),
                    (L.MPIX_Get_accumulate_local_plan_async,
                     (origin, result, target, h, H.as_c_int(op), None)),
                    (L.MPIX_Get_accumulate_local_plan, (origin, result, target, h, H.as_c_int(op)))):
        out.append(f(*args))
        assert L.MPIX_Redop_last_error() == out[-1]
    return tuple(out)


def fetch(h, origin, result, target, op=H.MPI_SUM):
    r = launches(h, origin, result, target, op)
    assert r[2] == r[3]
    return r[2]


def reduce(h, source, target, op=H.MPI_SUM):
    r = launches(h, source, B, target, op)
    assert r[0] == r[1]
    return r[0]


@pytest.fixture()
def plans():
    made = []

    def make(*a, **k):
        made.append(plan_of(*a, **k))
        return made[-1]
    yield make
    for h in made:
        assert R.lib().MPIX_Iov_plan_free(ctypes.byref(h)) == 0


def test_null_plan_then_op(plans):
    assert launches(None, None, None, None, 0x18000000) == (H.MPI_ERR_ARG,) * 4
    h = plans([96, -64], [4, 4])
    # the op before the buffers
    for op in (0x18000000, H.MPI_BAND, H.MPI_MAXLOC, H.MPIX_EQUAL):
        assert launches(h, None, None, None, op) == (H.MPI_ERR_OP,) * 4
    hb = plans([0], [16], H.MPI_BYTE)
    assert launches(hb, A, B, C, H.MPIX_EQUAL) == (H.MPI_ERR_OP,) * 4
    # ... and before the zero-element shortcut
    h0 = plans([], [])
    assert launches(h0, None, None, None, H.MPI_BAND) == (H.MPI_ERR_OP,) * 4


def test_zero_element_plan_touches_nothing(plans):
    for h in (plans([], []), plans([0, 64, -8], [0, 0, 0])):
        for op in (H.MPI_SUM, H.MPI_NO_OP, H.MPI_REPLACE):
            assert launches(h, None, WILD, None, op) == (0,) * 4
            assert launches(h, WILD, None, WILD, op) == (0,) * 4


def test_null_buffers(plans):
    h = plans([96, -64], [4, 4])
    for bad in (None, WILD):
        assert fetch(h, bad, B, C) == H.MPI_ERR_BUFFER
        assert fetch(h, A, bad, C) == H.MPI_ERR_BUFFER
        assert fetch(h, A, B, bad) == H.MPI_ERR_BUFFER
        assert reduce(h, bad, C) == H.MPI_ERR_BUFFER
        assert reduce(h, A, bad) == H.MPI_ERR_BUFFER
        # the reduce form reads its source whatever the op (as the iov entry)
        assert reduce(h, bad, C, H.MPI_NO_OP) == H.MPI_ERR_BUFFER


def test_overlap_against_the_bounding_range_at_its_edges(plans):
    """MPI_ERR_BUFFER is also what a wild but disjoint triple ends in (the
    placement check), so the overlap arithmetic is pinned where the two differ:
    a legal pair without a kernel is MPI_ERR_TYPE only once the overlap check
    has passed.  bf16 runs of 4 elements at bytes 96 and -64: packed 16 bytes,
    bounding range [T - 64, T + 104)."""
    T, op = B, H.MPI_MAX
    h = plans([96, -64], [4, 4], H.MPIX_BFLOAT16)
    assert fetch(h, A, C, T, op) == H.MPI_ERR_TYPE
    assert reduce(h, A, T, op) == H.MPI_ERR_TYPE
    for z in (T - 80, T + 104):                 # touching, not overlapping
        assert fetch(h, A, z, T, op) == H.MPI_ERR_TYPE
        assert fetch(h, z, C, T, op) == H.MPI_ERR_TYPE
        assert reduce(h, z, T, op) == H.MPI_ERR_TYPE
    for z in (T - 79, T - 64, T, T + 50, T + 103):      # the gap between the runs included
        assert fetch(h, A, z, T, op) == H.MPI_ERR_BUFFER
        assert fetch(h, z, C, T, op) == H.MPI_ERR_BUFFER
        assert reduce(h, z, T, op) == H.MPI_ERR_BUFFER
    assert fetch(h, A, A + 15, T, op) == H.MPI_ERR_BUFFER       # origin / result
    assert fetch(h, A, A + 16, T, op) == H.MPI_ERR_TYPE
    assert fetch(h, A, C, T, H.MPI_PROD) == H.MPI_ERR_TYPE
    # MPI_NO_OP ignores the origin altogether: inside the range, and NULL
    hd = plans([96, -64], [4, 4])
    assert fetch(hd, T, C, T, H.MPI_NO_OP) == H.MPI_ERR_BUFFER   # placement, not overlap ...
    assert fetch(h, T, C, T, H.MPI_NO_OP) == H.MPI_ERR_BUFFER
    # a single-run plan checks the same way
    h1 = plans([32], [4], H.MPIX_BFLOAT16)      # [T + 32, T + 40), packed 8
    assert fetch(h1, A, T + 24, T, op) == H.MPI_ERR_TYPE
    assert fetch(h1, A, T + 25, T, op) == H.MPI_ERR_BUFFER
    assert fetch(h1, A, T + 39, T, op) == H.MPI_ERR_BUFFER
    assert fetch(h1, A, T + 40, T, op) == H.MPI_ERR_TYPE
    assert fetch(h1, A, T, T, op) == H.MPI_ERR_TYPE             # below the run: no overlap


def test_placement_is_a_buffer_error_and_prepare_needs_a_gpu(plans):
    """valid arguments on wild pointers get as far as the placement check;
    without a GPU prepare fails and leaves the plan usable"""
    import torch
    for h in (plans([96, -64], [4, 4]), plans([8], [40])):
        for op in (H.MPI_SUM, H.MPI_REPLACE, H.MPI_NO_OP):
            assert launches(h, A, B, C, op) == (H.MPI_ERR_BUFFER,) * 4
        assert fetch(h, None, B, C, H.MPI_NO_OP) == H.MPI_ERR_BUFFER
    h = plans([96, -64], [4, 4])
    if not torch.cuda.is_available():
        assert R.lib().MPIX_Iov_plan_prepare(h, -1) != 0
        assert R.lib().MPIX_Iov_plan_prepare(h, 0) != 0
    v = [AINT() for _ in range(6)]
    assert R.lib().MPIX_Iov_plan_info(h, *[ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [8, 2, 1, -64, 128, 7 * 8 + 2 * 4]


def test_every_pair_with_a_fetch_iov_kernel_has_plan_kernels(plans):
    types = sorted({v for k, v in vars(H).items()
                    if k.startswith(('MPI_', 'MPIX_', 'MPIR_')) and isinstance(v, int)
                    and (v >> 24) in (0x4c, 0x8c)})
    ops = [H.MPI_MAX, H.MPI_MIN, H.MPI_SUM, H.MPI_PROD, H.MPI_LAND, H.MPI_BAND, H.MPI_LOR,
           H.MPI_BOR, H.MPI_LXOR, H.MPI_BXOR, H.MPI_MINLOC, H.MPI_MAXLOC]
    covered = 0
    for dt in types:
        ext = R.datatype_extent(dt)
        if ext <= 0:
            continue
        h = plans([0, 4 * ext], [1, 1], dt)
        for op in ops:
            if not R.internal_op_dt_check(op, R.datatype_internal(dt)):
                assert launches(h, A, B, C, op) == (H.MPI_ERR_OP,) * 4
                continue
            iov = R.lib().MPIX_Get_accumulate_local_iov_async(
                A, B, C, 2, tab([0, 4 * ext]), tab([1, 1]), H.as_c_int(dt), H.as_c_int(op), None)
            assert iov in (H.MPI_ERR_BUFFER, H.MPI_ERR_TYPE)
            assert launches(h, A, B, C, op) == (iov,) * 4, (hex(dt), hex(op))
            covered += iov == H.MPI_ERR_BUFFER
    assert covered > 300


def test_single_run_plans_agree_with_the_contiguous_entries(plans):
    """a plan of one run launches through the contiguous entries' tables, while
    its MPI_ERR_TYPE check reads the plan kernels' table: pair by pair both
    must say what the contiguous tables hold: MPIX_Redop_has_gpu_path for the
    reduce form's (MPIX_Reduce_local_async itself looks at placement before the
    kernel, so wild pointers cannot ask it), MPIX_Get_accumulate_local_async's
    own error class for the fetch form's"""
    L = R.lib()
    types = sorted({v for k, v in vars(H).items()
                    if k.startswith(('MPI_', 'MPIX_', 'MPIR_')) and isinstance(v, int)
                    and (v >> 24) in (0x4c, 0x8c)})
    ops = [H.MPI_MAX, H.MPI_MIN, H.MPI_SUM, H.MPI_PROD, H.MPI_LAND, H.MPI_BAND, H.MPI_LOR,
           H.MPI_BOR, H.MPI_LXOR, H.MPI_BXOR, H.MPI_MINLOC, H.MPI_MAXLOC]
    covered = declined = 0
    for dt in types:
        ext = R.datatype_extent(dt)
        if ext <= 0:
            continue
        h = plans([0, 2 * ext], [2, 1], dt)         # adjacent: one run of three elements
        v = AINT()
        assert L.MPIX_Iov_plan_info(h, None, ctypes.byref(v), None, None, None, None) == 0
        assert v.value == 1
        for op in ops:
            fetch_rc = L.MPIX_Get_accumulate_local_async(A, B, C, 3, H.as_c_int(dt),
                                                         H.as_c_int(op), None)
            if not R.internal_op_dt_check(op, R.datatype_internal(dt)):
                reduce_rc = H.MPI_ERR_OP
            else:
                reduce_rc = H.MPI_ERR_BUFFER if R.has_gpu_path(op, dt) else H.MPI_ERR_TYPE
            assert launches(h, A, B, C, op) == (reduce_rc, reduce_rc, fetch_rc, fetch_rc), \
                (hex(dt), hex(op))
            assert reduce_rc == fetch_rc, (hex(dt), hex(op))
            covered += reduce_rc == H.MPI_ERR_BUFFER
            declined += reduce_rc == H.MPI_ERR_TYPE
    assert covered > 300 and declined >= 2          # bf16 MAX / MIN / PROD at the least


# ------------------------------------------------------------- no HIP call
def test_create_info_free_make_no_hip_call(shim):  # noqa: F811
    calls = '\n'.join([
        'T = a * 4; P = ctypes.POINTER(a); DOUBLE, DOUBLE_INT = 0x4c00080b, 0x8c000001',
        'L.MPIX_Iov_plan_create.argtypes = [a, P, P, i, ctypes.POINTER(vp)]',
        'L.MPIX_Iov_plan_create_iovec.argtypes = [a, P, P, i, ctypes.POINTER(vp)]',
        'L.MPIX_Iov_plan_info.argtypes = [vp] + [P] * 6',
        'L.MPIX_Iov_plan_free.argtypes = [ctypes.POINTER(vp)]',
        'h = vp()',
        'assert L.MPIX_Iov_plan_create(4, T(0, 84, 160, 244), T(4, 4, 4, 4), DOUBLE,'
        ' ctypes.byref(h)) == 0 and h.value',
        'v = [a() for _ in range(6)]',
        'assert L.MPIX_Iov_plan_info(h, *[ctypes.byref(x) for x in v]) == 0',
        'assert [x.value for x in v][:3] == [16, 4, 2], [x.value for x in v]',
        'assert L.MPIX_Iov_plan_free(ctypes.byref(h)) == 0 and not h.value',
        'assert L.MPIX_Iov_plan_create_iovec(4, T(0, 8, 16, 24), T(8, 4, 8, 4), DOUBLE_INT,'
        ' ctypes.byref(h)) == 0 and h.value',
        'assert L.MPIX_Iov_plan_info(h, *[ctypes.byref(x) for x in v]) == 0',
        'assert [x.value for x in v][:3] == [2, 1, 1], [x.value for x in v]',
        'assert L.MPIX_Iov_plan_free(ctypes.byref(h)) == 0',
        'assert L.MPIX_Iov_plan_create(1, T(2, 0, 0, 0), T(4, 0, 0, 0), DOUBLE,'
        ' ctypes.byref(h)) == 12 and not h.value        # MPI_ERR_ARG',
        # a launch refused by a check that needs no device makes none either
        'L.MPIX_Reduce_local_plan_async.argtypes = [vp, vp, vp, i, vp]',
        'assert L.MPIX_Reduce_local_plan_async(None, None, None, SUM, None) == 12',
        'assert L.MPIX_Iov_plan_create(0, None, None, DOUBLE, ctypes.byref(h)) == 0',
        'assert L.MPIX_Reduce_local_plan_async(None, None, h, SUM, None) == 0',
        'assert L.MPIX_Iov_plan_free(ctypes.byref(h)) == 0',
    ])
    hits, last = _probe(shim, calls)
    assert hits == 0, 'HIP entered through %s' % last


def test_positive_control_prepare_is_intercepted(shim):  # noqa: F811
    calls = '\n'.join([
        'T = a * 2; P = ctypes.POINTER(a)',
        'L.MPIX_Iov_plan_create.argtypes = [a, P, P, i, ctypes.POINTER(vp)]',
        'L.MPIX_Iov_plan_prepare.argtypes = [vp, i]',
        'h = vp()',
        'assert L.MPIX_Iov_plan_create(2, T(0, 80), T(4, 4), 0x4c00080b, ctypes.byref(h)) == 0',
        'assert L.MPIX_Iov_plan_prepare(h, 0) != 0',
    ])
    hits, last = _probe(shim, calls)
    assert hits > 0 and last.startswith('hip'), (hits, last)


# ---------------------------------------------------- the built code objects
UNITS = ['inst_plan_%s.o' % u for u in ('int', 'fp', 'pair')] + ['inst_plan_copy.o']
REDUCE, FETCH, COPY = '_ZN4mpix13k_plan_reduceI', '_ZN4mpix13k_plan_getaccI', \
    '_ZN4mpix11k_plan_copyI'
PARAMS = 'EvPKNT_4unitE'


@pytest.fixture(scope='module')
def kernels():
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip('ROCm llvm tools not found')
    objs = [os.path.join(BUILD, u) for u in UNITS]
    if not all(os.path.exists(o) for o in objs):
        pytest.skip('library objects not built (run __graft_entry__.build())')
    return {u: _kernels(o) for u, o in zip(UNITS, objs)}


def test_new_units_hold_only_the_new_kernel_families(kernels):
    """one reduce and one fetch kernel per combiner of the fetch-iov units, the
    copy kernel per unit body and mode"""
    for u in ('int', 'fp', 'pair'):
        names = [k[0] for k in kernels['inst_plan_%s.o' % u]]
        assert all(n.startswith((REDUCE, FETCH)) for n in names), \
            [n for n in names if not n.startswith((REDUCE, FETCH))][:3]
        iov = [k[0] for k in _kernels(os.path.join(BUILD, 'inst_getacc_iov_%s.o' % u))]
        # the same combiners: the template argument, up to the parameter list
        # (every one of these kernels takes `const typename C::unit *` first)
        def combiners(ns, prefix):
            assert all(PARAMS in n for n in ns)
            return sorted(n[len(prefix):n.index(PARAMS)] for n in ns)
        comb = combiners(iov, '_ZN4mpix12k_getacc_iovI')
        assert combiners([n for n in names if n.startswith(REDUCE)], REDUCE) == comb
        assert combiners([n for n in names if n.startswith(FETCH)], FETCH) == comb
        assert len(set(comb)) == len(comb)
        assert len(comb) >= 30
    other = [k[0] for k in kernels[UNITS[3]]]
    assert all(n.startswith(COPY) for n in other), other
    assert len(other) == 3 * 9          # 3 modes x (6 raw units, 3 padded pairs)


def test_new_kernels_use_no_scratch_and_no_hidden_arguments(kernels):
    ks = [k for u in UNITS for k in kernels[u]]
    assert len(ks) > 200
    assert not [(n, p) for n, _, p, _ in ks if p][:5]
    assert not [n for n, _, _, k in ks if k < 0][:5]


# ------------------------------------------------------- the Python mirror
def test_python_mirror_range_checks():
    tgt, pk = np.zeros(11, np.float64), np.zeros(5, np.float64)
    short = np.zeros(4, np.float64)
    with R.IovPlan.from_iov([16, 64], [2, 3], H.MPI_DOUBLE) as p:   # target [16, 88), packed 40
        assert p.info()['hi_byte'] == 88
        for bufs in ((short, pk, tgt), (pk, short, tgt), (pk, pk.copy(), np.zeros(10, np.float64))):
            with pytest.raises(ValueError):
                R.get_accumulate_local_plan(*bufs, p, H.MPI_SUM, stream=0)
            with pytest.raises(ValueError):
                R.get_accumulate_local_plan(*bufs, p, H.MPI_SUM, sync=True)
        with pytest.raises(ValueError):         # origin=None: the other two are still checked
            R.get_accumulate_local_plan(None, short, tgt, p, H.MPI_NO_OP, stream=0)
        for bufs in ((short, tgt), (pk, np.zeros(10, np.float64))):
            with pytest.raises(ValueError):
                R.reduce_local_plan(*bufs, p, H.MPI_SUM, stream=0)
        # in range: the C call then refuses the pageable operands
        assert R.get_accumulate_local_plan(pk, pk.copy(), tgt, p, H.MPI_SUM,
                                           stream=0) == H.MPI_ERR_BUFFER
        assert R.reduce_local_plan(pk, tgt, p, H.MPI_SUM, stream=0) == H.MPI_ERR_BUFFER
    with pytest.raises(ValueError):             # closed
        R.reduce_local_plan(pk, tgt, p, H.MPI_SUM, stream=0)
    with R.IovPlan.from_iovec([-16, 48], [16, 24], H.MPI_DOUBLE) as p:
        assert (p.info()['lo_byte'], p.info()['hi_byte']) == (-16, 72)
        with pytest.raises(ValueError):         # the lowest run byte lies before the buffer
            R.reduce_local_plan(pk, tgt[1:], p, H.MPI_SUM, stream=0)
        # a negative offset inside the storage of a view passes the mirror
        assert R.reduce_local_plan(pk, tgt[2:], p, H.MPI_SUM, stream=0) == H.MPI_ERR_BUFFER
    with pytest.raises(R.RedopError) as e:
        R.IovPlan.from_iov([2], [4], H.MPI_DOUBLE)
    assert e.value.code == H.MPI_ERR_ARG
    with pytest.raises(ValueError):
        R.IovPlan.from_iov([0, 8], [4], H.MPI_DOUBLE)


def test_package_exports():
    import mpich_amd
    assert mpich_amd.IovPlan is R.IovPlan
    assert mpich_amd.reduce_local_plan is R.reduce_local_plan
    assert mpich_amd.get_accumulate_local_plan is R.get_accumulate_local_plan
