"""Typed accumulate / get-accumulate (MPIX_[Get_]accumulate_local_typed*,
MPIX_Iov_plan_locate / _prepare_packed / _info_packed) on a machine without a
GPU: the packed-order lookup against a naive walk of the merged runs for every
packed index, the size of the packed-order table as a closed form, that
MPIX_Iov_plan_info reports what it did, the entries' check order on wild
pointers, that none of this makes a HIP call, what the new instantiation units
hold, and the Python mirror's range checks.

Wild pointers stand for buffers: a call that is refused, or that has nothing
to do, never looks at them."""
import ctypes
import os

import numpy as np
import pytest

from mpich_amd import handles as H
from mpich_amd import redop as R
from tests.test_getacc_iov_cpu import A, AINT, B, C, WILD
from tests.test_kernel_resources import BUILD, OBJDUMP, READELF, _kernels
from tests.test_no_hip_init import _probe, shim  # noqa: F401  (shim is a fixture)
from tests.test_plan_cpu import create

TILE_LENS = [255, 1, 1, 255, 300, 5]


# ------------------------------------------------------------------- locate
def merged(offs, cnts, ext):
    """the merged runs of a table, restated: empty runs dropped, a run joins
    its predecessor in call order when it starts where that one ends"""
    m = []
    for o, c in zip(offs, cnts):
        if c == 0:
            continue
        if m and m[-1][0] + m[-1][1] * ext == o:
            m[-1][1] += c
        else:
            m.append([o, c])
    return m


def walk(offs, cnts, ext):
    """byte offset of every packed index, by walking the runs"""
    return [o + k * ext for o, c in merged(offs, cnts, ext) for k in range(c)]


def packed_bytes(runs, elements):
    return 0 if runs <= 1 else (2 * runs + 1) * 8 + ((elements + 255) // 256 + 1) * 4


def locate_all(p, n):
    L, h, v = R.lib(), p.handle, AINT()
    out = []
    for k in range(n):
        assert L.MPIX_Iov_plan_locate(h, k, ctypes.byref(v)) == 0
        out.append(v.value)
    return out


def gapped(lens, ext, gap=3, start=0):
    offs, pos = [], start
    for n in lens:
        pos += gap
        offs.append(pos * ext)
        pos += n
    return offs


def check_locate(offs, cnts, dt, ext, runs=None):
    want = walk(offs, cnts, ext)
    with R.IovPlan.from_iov(offs, cnts, dt) as p:
        i = p.info()
        assert i['elements'] == len(want)
        if runs is not None:
            assert i['runs'] == runs
        assert locate_all(p, len(want)) == want
        assert p.info_packed() == packed_bytes(i['runs'], i['elements'])
        assert [p.locate(k) for k in (0, len(want) - 1)] == [want[0], want[-1]]
        v = AINT(77)
        for bad in (-1, len(want), len(want) + 256, 1 << 60):
            assert R.lib().MPIX_Iov_plan_locate(p.handle, bad, ctypes.byref(v)) == H.MPI_ERR_COUNT
            assert R.lib().MPIX_Redop_last_error() == H.MPI_ERR_COUNT
        assert v.value == 77


def test_locate_tile_edges():
    """run starts at packed indices 255, 256, 257 and 512, a partial last tile;
    three of it in a row; its reverse"""
    for lens in (TILE_LENS, TILE_LENS * 3, TILE_LENS[::-1], [256, 1, 560], [256, 256, 256]):
        check_locate(gapped(lens, 8), lens, H.MPI_DOUBLE, 8, runs=len(lens))


def test_locate_one_run():
    check_locate([24], [700], H.MPI_DOUBLE, 8, runs=1)
    check_locate([-40, -8, 16], [4, 3, 2], H.MPI_DOUBLE, 8, runs=1)         # merged into one
    with R.IovPlan.from_iov([-40, -8, 16], [4, 3, 2], H.MPI_DOUBLE) as p:
        assert p.info_packed() == 0 and p.locate(0) == -40 and p.locate(8) == 24


def test_locate_two_residues_and_negative_offsets():
    rng = np.random.default_rng(0x5EED1201)
    lens = [int(x) for x in rng.integers(0, 40, 60)]
    lens[5], lens[30] = 300, 513
    slots = gapped(lens, 8, gap=4, start=-2000)
    order = rng.permutation(len(lens))
    offs = [slots[j] + (4 if i % 3 == 1 else 0) for i, j in enumerate(order)]
    cnts = [lens[j] for j in order]
    assert min(offs) < 0 < max(offs) and {o % 8 for o, c in zip(offs, cnts) if c} == {0, 4}
    with R.IovPlan.from_iov(offs, cnts, H.MPI_DOUBLE) as p:
        assert p.info()['groups'] == 2
    check_locate(offs, cnts, H.MPI_DOUBLE, 8)
    check_locate([2 * o for o in offs], cnts, H.MPI_INT16_T, 2)     # a 2-byte type's residues


def test_locate_double_int_iovec_merges_to_one_run():
    offs, lens = [], []
    for k in range(37):
        offs += [32 + 16 * k, 32 + 16 * k + 8]
        lens += [8, 4]
    with R.IovPlan.from_iovec(offs, lens, H.MPI_DOUBLE_INT) as p:
        assert p.info()['runs'] == 1 and p.info_packed() == 0
        assert locate_all(p, 37) == [32 + 16 * k for k in range(37)]
    # with a hole after element 20: two runs, a table
    offs = [o + (64 if o >= 32 + 16 * 21 else 0) for o in offs]
    with R.IovPlan.from_iovec(offs, lens, H.MPI_DOUBLE_INT) as p:
        assert p.info()['runs'] == 2 and p.info_packed() == packed_bytes(2, 37)
        assert locate_all(p, 37) == [32 + 16 * k + (64 if k >= 21 else 0) for k in range(37)]


def test_locate_ten_thousand_runs_of_one():
    n = 10 ** 4
    offs = [16 * (n - k) for k in range(n)]         # descending: nothing merges
    check_locate(offs, [1] * n, H.MPI_DOUBLE, 8, runs=n)


def test_locate_and_info_packed_argument_errors():
    L, v = R.lib(), AINT(5)
    assert L.MPIX_Iov_plan_locate(None, 0, ctypes.byref(v)) == H.MPI_ERR_ARG
    assert L.MPIX_Iov_plan_info_packed(None, ctypes.byref(v)) == H.MPI_ERR_ARG
    assert L.MPIX_Iov_plan_prepare_packed(None, 0) == H.MPI_ERR_ARG
    assert L.MPIX_Redop_last_error() == H.MPI_ERR_ARG
    with R.IovPlan.from_iov([0, 80], [4, 4], H.MPI_DOUBLE) as p:
        assert L.MPIX_Iov_plan_locate(p.handle, 0, None) == H.MPI_ERR_ARG
        assert L.MPIX_Iov_plan_locate(p.handle, 99, None) == H.MPI_ERR_ARG      # before the index
        assert L.MPIX_Iov_plan_info_packed(p.handle, None) == 0
    with R.IovPlan.from_iov([], [], H.MPI_DOUBLE) as p:
        assert p.info_packed() == 0
        assert L.MPIX_Iov_plan_locate(p.handle, 0, ctypes.byref(v)) == H.MPI_ERR_COUNT
    assert v.value == 5


def test_plan_info_is_what_it_was():
    """the numbers tests/test_plan_cpu.py pins, beside the new table's size"""
    def both(offs, cnts):
        with R.IovPlan.from_iov(offs, cnts, H.MPI_DOUBLE) as p:
            return p.info(), p.info_packed()
    i, pk = both([32, 0], [4, 4])
    assert i['table_bytes'] == 7 * 8 + 2 * 4 and pk == 5 * 8 + 2 * 4
    i, pk = both([0, 84, 160, 244], [4, 4, 4, 4])
    assert i['table_bytes'] == 2 * (7 * 8 + 2 * 4) and pk == 9 * 8 + 2 * 4
    i, pk = both([0, 8000], [300, 400])
    assert i['table_bytes'] == 7 * 8 + 4 * 4 and pk == 5 * 8 + 4 * 4
    i, pk = both([96, -64], [4, 4])
    assert i == dict(elements=8, runs=2, groups=1, lo_byte=-64, hi_byte=128,
                     table_bytes=7 * 8 + 2 * 4)
    i, pk = both([0, 32, 64], [4, 4, 2])
    assert i['table_bytes'] == 0 and pk == 0


# -------------------------------------------------------------- check order
def plan_of(offs, cnts, dt=H.MPI_DOUBLE):
    rc, h = create(offs, cnts, dt)
    assert rc == 0
    return h


@pytest.fixture()
def plans():
    made = []

    def make(*a, **k):
        made.append(plan_of(*a, **k))
        return made[-1]
    yield make
    for h in made:
        assert R.lib().MPIX_Iov_plan_free(ctypes.byref(h)) == 0


def calls(o, op_, r, rp, t, tp, op=H.MPI_SUM):
    """(accumulate async, accumulate sync, fetch async, fetch sync)"""
    L, cop = R.lib(), H.as_c_int(op)
    out = []
    for f, args in ((L.MPIX_Accumulate_local_typed_async, (o, op_, t, tp, cop, None)),
                    (L.MPIX_Accumulate_local_typed, (o, op_, t, tp, cop)),
                    (L.MPIX_Get_accumulate_local_typed_async, (o, op_, r, rp, t, tp, cop, None)),
                    (L.MPIX_Get_accumulate_local_typed, (o, op_, r, rp, t, tp, cop))):
        out.append(f(*args))
        assert L.MPIX_Redop_last_error() == out[-1]
    return tuple(out)


def fetch(*a, **k):
    r = calls(*a, **k)
    assert r[2] == r[3]
    return r[2]


def acc(o, op_, t, tp, op=H.MPI_SUM):
    r = calls(o, op_, B, None, t, tp, op)
    assert r[0] == r[1]
    return r[0]


def test_check_1_null_target_plan_before_the_op(plans):
    h = plans([96, -64], [4, 4])
    assert calls(A, h, B, h, C, None, 0x18000000) == (H.MPI_ERR_ARG,) * 4
    assert calls(None, None, None, None, None, None, H.MPI_BAND) == (H.MPI_ERR_ARG,) * 4


def test_check_2_op_before_the_plans_types(plans):
    h, hf = plans([96, -64], [4, 4]), plans([96, -64], [4, 4], H.MPI_FLOAT)
    for op in (0x18000000, H.MPI_BAND, H.MPI_MAXLOC, H.MPIX_EQUAL):
        assert calls(A, hf, B, hf, C, h, op) == (H.MPI_ERR_OP,) * 4
    hb = plans([0], [16], H.MPI_BYTE)
    assert calls(A, hf, B, hf, C, hb, H.MPIX_EQUAL) == (H.MPI_ERR_OP,) * 4
    h0 = plans([], [])
    assert calls(None, None, None, None, None, h0, H.MPI_BAND) == (H.MPI_ERR_OP,) * 4


def test_check_3_type_then_count_before_zero_elements_and_buffers(plans):
    h = plans([96, -64], [4, 4])
    hf = plans([96, -64], [4, 4], H.MPI_FLOAT)          # another type, the same count
    h9 = plans([96, -64], [4, 5])                       # the same type, another count
    hf9 = plans([96, -64], [4, 5], H.MPI_FLOAT)         # both: the type is looked at first
    h0 = plans([], [])
    for bad, code in ((hf, H.MPI_ERR_TYPE), (h9, H.MPI_ERR_COUNT), (hf9, H.MPI_ERR_TYPE)):
        # NULL buffers (check 5) as well
        assert calls(None, bad, None, h, None, h) == (code,) * 4
        assert fetch(None, h, None, bad, None, h) == code
        assert acc(None, h, None, h) == H.MPI_ERR_BUFFER
    # the origin's plan before the result's
    assert fetch(None, hf, None, h9, None, h) == H.MPI_ERR_TYPE
    assert fetch(None, h9, None, hf, None, h) == H.MPI_ERR_COUNT
    # a zero-element target (check 4) does not excuse a mismatch
    assert calls(WILD, h, WILD, h, WILD, h0) == (H.MPI_ERR_COUNT,) * 4
    assert fetch(WILD, h0, WILD, hf, WILD, h0) == H.MPI_ERR_TYPE
    # under MPI_NO_OP the origin's plan is not examined, the result's is
    assert fetch(None, hf9, None, h, None, h, H.MPI_NO_OP) == H.MPI_ERR_BUFFER
    assert fetch(None, hf9, None, h9, None, h, H.MPI_NO_OP) == H.MPI_ERR_COUNT
    assert acc(None, hf9, None, h0, H.MPI_NO_OP) == 0


def test_check_4_zero_elements_touch_nothing(plans):
    h0, hz = plans([], []), plans([0, 64, -8], [0, 0, 0])
    for op in (H.MPI_SUM, H.MPI_NO_OP, H.MPI_REPLACE):
        assert calls(WILD, h0, None, hz, WILD, h0, op) == (0,) * 4
        assert calls(None, None, WILD, None, None, hz, op) == (0,) * 4


def test_check_5_missing_operands_before_overlap_and_kernel(plans):
    """bf16 MAX is a legal pair without a kernel (check 7, MPI_ERR_TYPE)"""
    hb = plans([96, -64], [4, 4], H.MPIX_BFLOAT16)
    T = C
    for bad in (None, WILD):
        assert fetch(bad, hb, T, hb, T, hb, H.MPI_MAX) == H.MPI_ERR_BUFFER
        assert fetch(T, hb, bad, hb, T, hb, H.MPI_MAX) == H.MPI_ERR_BUFFER
        assert fetch(T, hb, T, hb, bad, hb, H.MPI_MAX) == H.MPI_ERR_BUFFER
        assert acc(bad, hb, T, hb, H.MPI_MAX) == H.MPI_ERR_BUFFER
        assert acc(T, hb, bad, hb, H.MPI_MAX) == H.MPI_ERR_BUFFER
    assert fetch(A, hb, B, hb, C, hb, H.MPI_MAX) == H.MPI_ERR_TYPE


def test_check_6_bounding_ranges_at_their_edges_before_the_kernel(plans):
    """bf16 runs of 4 elements at bytes 96 and -64: every derived side covers
    [P - 64, P + 104), a packed one [P, P + 16).  MPI_ERR_TYPE (check 7) shows
    that the overlap check has passed."""
    op = H.MPI_MAX
    hb = plans([96, -64], [4, 4], H.MPIX_BFLOAT16)
    T = B
    assert fetch(A, hb, C, hb, T, hb, op) == H.MPI_ERR_TYPE
    for z in (T - 168, T + 168):            # touching, not overlapping
        assert fetch(A, hb, z, hb, T, hb, op) == H.MPI_ERR_TYPE
        assert fetch(z, hb, C, hb, T, hb, op) == H.MPI_ERR_TYPE
        assert acc(z, hb, T, hb, op) == H.MPI_ERR_TYPE
    for z in (T - 167, T, T + 20, T + 167):     # gaps included: interleaved layouts are refused
        assert fetch(A, hb, z, hb, T, hb, op) == H.MPI_ERR_BUFFER
        assert fetch(z, hb, C, hb, T, hb, op) == H.MPI_ERR_BUFFER
        assert acc(z, hb, T, hb, op) == H.MPI_ERR_BUFFER
    # origin against result, one derived and one packed: [A - 64, A + 104) and [z, z + 16)
    for z, code in ((A - 80, H.MPI_ERR_TYPE), (A - 79, H.MPI_ERR_BUFFER),
                    (A + 50, H.MPI_ERR_BUFFER), (A + 103, H.MPI_ERR_BUFFER),
                    (A + 104, H.MPI_ERR_TYPE)):
        assert fetch(A, hb, z, None, T, hb, op) == code
        assert fetch(z, None, A, hb, T, hb, op) == code
    # both packed: the plan entries' rule
    assert fetch(A, None, A + 15, None, T, hb, op) == H.MPI_ERR_BUFFER
    assert fetch(A, None, A + 16, None, T, hb, op) == H.MPI_ERR_TYPE
    # a packed origin inside the target's gap; a one-run plan's range starts at its offset
    assert acc(T + 20, None, T, hb, op) == H.MPI_ERR_BUFFER
    h1 = plans([32], [4], H.MPIX_BFLOAT16)      # [P + 32, P + 40)
    assert acc(T + 24 - 32, h1, T, h1, op) == H.MPI_ERR_TYPE
    assert acc(T + 25 - 32, h1, T, h1, op) == H.MPI_ERR_BUFFER
    assert acc(T, None, T, h1, op) == H.MPI_ERR_TYPE
    # MPI_NO_OP ignores the origin altogether: on the target, NULL, and a garbage plan
    hd = plans([96, -64], [4, 4])
    junk = ctypes.c_void_p(0xdead0)
    for o, oplan in ((T, hd), (None, None), (None, junk), (WILD, junk)):
        assert fetch(o, oplan, C, hd, T, hd, H.MPI_NO_OP) == H.MPI_ERR_BUFFER   # placement
        assert fetch(o, oplan, T + 20, hd, T, hd, H.MPI_NO_OP) == H.MPI_ERR_BUFFER
    h0 = plans([], [])
    assert fetch(None, junk, None, h0, None, h0, H.MPI_NO_OP) == 0
    assert acc(None, junk, None, h0, H.MPI_NO_OP) == 0


def test_check_7_kernel_before_placement_and_8_placement(plans):
    hb = plans([96, -64], [4, 4], H.MPIX_BFLOAT16)
    h, h1 = plans([96, -64], [4, 4]), plans([8], [8])
    for op in (H.MPI_MAX, H.MPI_MIN, H.MPI_PROD):
        assert calls(A, hb, B, None, C, hb, op) == (H.MPI_ERR_TYPE,) * 4
    # valid arguments on wild pointers get as far as the placement check
    for op in (H.MPI_SUM, H.MPI_REPLACE):
        assert calls(A, hb, B, hb, C, hb, op) == (H.MPI_ERR_BUFFER,) * 4
        for o, r, t in ((h, h, h), (None, h, h1), (h1, None, h), (h1, h1, h1), (None, None, h)):
            assert calls(A, o, B, r, C, t, op) == (H.MPI_ERR_BUFFER,) * 4
    assert fetch(None, None, B, h, C, h, H.MPI_NO_OP) == H.MPI_ERR_BUFFER
    assert acc(None, None, C, h, H.MPI_NO_OP) == H.MPI_ERR_BUFFER       # the target is placed


def test_every_pair_with_plan_kernels_has_typed_kernels(plans):
    types = sorted({v for k, v in vars(H).items()
                    if k.startswith(('MPI_', 'MPIX_', 'MPIR_')) and isinstance(v, int)
                    and (v >> 24) in (0x4c, 0x8c)})
    ops = [H.MPI_MAX, H.MPI_MIN, H.MPI_SUM, H.MPI_PROD, H.MPI_LAND, H.MPI_BAND, H.MPI_LOR,
           H.MPI_BOR, H.MPI_LXOR, H.MPI_BXOR, H.MPI_MINLOC, H.MPI_MAXLOC]
    L, covered = R.lib(), 0
    for dt in types:
        ext = R.datatype_extent(dt)
        if ext <= 0:
            continue
        h = plans([0, 4 * ext], [1, 1], dt)
        for op in ops:
            want = L.MPIX_Get_accumulate_local_plan_async(A, B, C, h, H.as_c_int(op), None)
            assert want in (H.MPI_ERR_OP, H.MPI_ERR_BUFFER, H.MPI_ERR_TYPE)
            assert calls(A + 0x1000, h, B + 0x1000, h, C + 0x1000, h, op) == (want,) * 4, \
                (hex(dt), hex(op))
            covered += want == H.MPI_ERR_BUFFER
    assert covered > 300


# ------------------------------------------------------------- no HIP call
def test_create_locate_info_packed_make_no_hip_call(shim):  # noqa: F811
    calls_ = '\n'.join([
        'T = a * 4; P = ctypes.POINTER(a); DOUBLE = 0x4c00080b',
        'L.MPIX_Iov_plan_create.argtypes = [a, P, P, i, ctypes.POINTER(vp)]',
        'L.MPIX_Iov_plan_locate.argtypes = [vp, a, P]',
        'L.MPIX_Iov_plan_info_packed.argtypes = [vp, P]',
        'L.MPIX_Iov_plan_free.argtypes = [ctypes.POINTER(vp)]',
        'h = vp(); v = a()',
        'assert L.MPIX_Iov_plan_create(4, T(0, 84, 160, 244), T(4, 4, 4, 4), DOUBLE,'
        ' ctypes.byref(h)) == 0 and h.value',
        'assert L.MPIX_Iov_plan_locate(h, 9, ctypes.byref(v)) == 0 and v.value == 168',
        'assert L.MPIX_Iov_plan_locate(h, 16, ctypes.byref(v)) == 2      # MPI_ERR_COUNT',
        'assert L.MPIX_Iov_plan_info_packed(h, ctypes.byref(v)) == 0 and v.value == 9 * 8 + 2 * 4',
        # launches refused by a check that needs no device make none either
        'L.MPIX_Get_accumulate_local_typed_async.argtypes = [vp, vp, vp, vp, vp, vp, i, vp]',
        'L.MPIX_Accumulate_local_typed.argtypes = [vp, vp, vp, vp, i]',
        'assert L.MPIX_Get_accumulate_local_typed_async(None, h, None, h, None, None, SUM,'
        ' None) == 12',
        'assert L.MPIX_Get_accumulate_local_typed_async(None, h, None, h, None, h, SUM,'
        ' None) == 1',
        'assert L.MPIX_Accumulate_local_typed(4096, h, 4200, h, SUM) == 1   # overlap',
        'e = vp()',
        'assert L.MPIX_Iov_plan_create(0, None, None, DOUBLE, ctypes.byref(e)) == 0',
        'assert L.MPIX_Accumulate_local_typed(None, e, None, e, SUM) == 0',
        'assert L.MPIX_Accumulate_local_typed(None, h, None, e, SUM) == 2       # MPI_ERR_COUNT',
        'assert L.MPIX_Iov_plan_free(ctypes.byref(e)) == 0',
        'assert L.MPIX_Iov_plan_free(ctypes.byref(h)) == 0 and not h.value',
    ])
    hits, last = _probe(shim, calls_)
    assert hits == 0, 'HIP entered through %s' % last


def test_positive_control_prepare_packed_is_intercepted(shim):  # noqa: F811
    calls_ = '\n'.join([
        'T = a * 2; P = ctypes.POINTER(a)',
        'L.MPIX_Iov_plan_create.argtypes = [a, P, P, i, ctypes.POINTER(vp)]',
        'L.MPIX_Iov_plan_prepare_packed.argtypes = [vp, i]',
        'h = vp()',
        'assert L.MPIX_Iov_plan_create(2, T(0, 80), T(4, 4), 0x4c00080b, ctypes.byref(h)) == 0',
        'assert L.MPIX_Iov_plan_prepare_packed(h, 0) != 0',
    ])
    hits, last = _probe(shim, calls_)
    assert hits > 0 and last.startswith('hip'), (hits, last)


# ---------------------------------------------------- the built code objects
UNITS = ['inst_typed_%s.o' % u for u in ('int', 'fp', 'pair')] + ['inst_typed_copy.o']
ACC, FETCH, COPY = '_ZN4mpix11k_typed_accI', '_ZN4mpix14k_typed_getaccI', '_ZN4mpix12k_typed_copyI'
PARAMS = 'EvPKNT_4unitE'


@pytest.fixture(scope='module')
def kernels():
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip('ROCm llvm tools not found')
    objs = [os.path.join(BUILD, u) for u in UNITS]
    if not all(os.path.exists(o) for o in objs):
        pytest.skip('library objects not built (run __graft_entry__.build())')
    return {u: _kernels(o) for u, o in zip(UNITS, objs)}


def test_typed_units_hold_only_the_three_new_families(kernels):
    for u in ('int', 'fp', 'pair'):
        names = [k[0] for k in kernels['inst_typed_%s.o' % u]]
        assert all(n.startswith((ACC, FETCH)) for n in names), \
            [n for n in names if not n.startswith((ACC, FETCH))][:3]
        iov = [k[0] for k in _kernels(os.path.join(BUILD, 'inst_getacc_iov_%s.o' % u))]

        def combiners(ns, prefix):
            assert all(PARAMS in n for n in ns)
            return sorted(n[len(prefix):n.index(PARAMS)] for n in ns)
        comb = combiners(iov, '_ZN4mpix12k_getacc_iovI')
        assert combiners([n for n in names if n.startswith(ACC)], ACC) == comb
        assert combiners([n for n in names if n.startswith(FETCH)], FETCH) == comb
        assert len(set(comb)) == len(comb) and len(comb) >= 30
    other = [k[0] for k in kernels[UNITS[3]]]
    assert all(n.startswith(COPY) for n in other), other
    assert len(other) == 3 * 9          # 3 modes x (6 raw units, 3 padded pairs)


def test_typed_kernels_use_no_scratch_and_no_hidden_arguments(kernels):
    ks = [k for u in UNITS for k in kernels[u]]
    assert len(ks) > 200
    assert not [(n, p) for n, _, p, _ in ks if p][:5]
    assert not [n for n, _, _, k in ks if k < 0][:5]


# ------------------------------------------------------- the Python mirror
def test_python_mirror_range_checks():
    tgt, pk = np.zeros(11, np.float64), np.zeros(5, np.float64)
    short = np.zeros(4, np.float64)
    with R.IovPlan.from_iov([16, 64], [2, 3], H.MPI_DOUBLE) as p, \
            R.IovPlan.from_iov([-16, 24], [1, 4], H.MPI_DOUBLE) as q:
        assert (p.info()['hi_byte'], q.info()['lo_byte'], q.info()['hi_byte']) == (88, -16, 56)
        # packed operands (a None plan) against the target plan's packed bytes
        for bufs in ((short, None, pk, None, tgt), (pk, None, short, None, tgt),
                     (pk, None, pk.copy(), None, np.zeros(10, np.float64))):
            for sync in (False, True):
                with pytest.raises(ValueError):
                    R.get_accumulate_local_typed(*bufs, p, H.MPI_SUM, sync=sync, stream=0)
        # derived operands against their own plan's bounding range
        with pytest.raises(ValueError):         # the origin's highest byte
            R.get_accumulate_local_typed(np.zeros(10, np.float64), p, pk, None, tgt, p,
                                         H.MPI_SUM, stream=0)
        with pytest.raises(ValueError):         # the result's lowest byte lies before the buffer
            R.get_accumulate_local_typed(pk, None, tgt[1:], q, tgt.copy(), p, H.MPI_SUM, stream=0)
        with pytest.raises(ValueError):
            R.accumulate_local_typed(tgt[1:], q, tgt.copy(), p, H.MPI_SUM, stream=0)
        with pytest.raises(ValueError):
            R.accumulate_local_typed(pk, None, np.zeros(10, np.float64), p, H.MPI_SUM, sync=True)
        with pytest.raises(ValueError):         # MPI_NO_OP: result and target are still checked
            R.get_accumulate_local_typed(None, None, short, None, tgt, p, H.MPI_NO_OP, stream=0)
        # ... and the origin is not, however short
        assert R.get_accumulate_local_typed(short, q, pk, None, tgt, p, H.MPI_NO_OP,
                                            stream=0) == H.MPI_ERR_BUFFER
        # in range: the C call then refuses the pageable operands
        assert R.get_accumulate_local_typed(tgt[2:], q, tgt.copy()[2:], q, tgt.copy(), p,
                                            H.MPI_SUM, stream=0) == H.MPI_ERR_BUFFER
        assert R.accumulate_local_typed(pk, None, tgt, p, H.MPI_SUM, stream=0) == H.MPI_ERR_BUFFER
        assert R.accumulate_local_typed(pk, None, tgt, p, H.MPI_NO_OP, stream=0) == H.MPI_ERR_BUFFER
    with pytest.raises(ValueError):             # closed
        R.accumulate_local_typed(pk, None, tgt, p, H.MPI_SUM, stream=0)
    with pytest.raises(ValueError):
        p.locate(0)
    with R.IovPlan.from_iov([16, 64], [2, 3], H.MPI_DOUBLE) as p:
        with pytest.raises(R.RedopError) as e:
            p.locate(5)
        assert e.value.code == H.MPI_ERR_COUNT
        assert [p.locate(k) for k in range(5)] == [16, 24, 64, 72, 80]
        assert p.info_packed() == 5 * 8 + 2 * 4


def test_package_exports():
    import mpich_amd
    assert mpich_amd.accumulate_local_typed is R.accumulate_local_typed
    assert mpich_amd.get_accumulate_local_typed is R.get_accumulate_local_typed
    assert R.IovPlan.locate and R.IovPlan.prepare_packed and R.IovPlan.info_packed
