"""The element-atomic entries (MPIX_[Get_]accumulate_local_atomic*,
MPIX_Compare_and_swap_local_atomic*, MPIX_Accumulate_atomic_is_supported) on a
machine without a GPU: the symbols in the header, the library and the Python
mirror, the predicate against a restatement over the oracle's tables, every
argument error in getacc_validate's order, that none of them makes a HIP call,
and the private segment of the new kernels read from the built code objects.

Wild pointers stand for buffers: a call that is refused, or that has nothing
to do, never looks at them."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import mpich_amd
from mpich_amd import handles as H
from mpich_amd import redop as R
from oracle import oracle as orc
from tests.test_kernel_resources import BUILD, OBJDUMP, READELF, ROOT, _kernels
from tests.test_no_hip_init import LIB, _probe, shim  # noqa: F401  (shim is a fixture)

A, B, C, D = 0x100000, 0x200000, 0x300000, 0x400000     # disjoint "buffers", never dereferenced
WILD = ctypes.c_void_p(-1).value

ENTRIES = ['MPIX_Accumulate_local_atomic', 'MPIX_Accumulate_local_atomic_async',
           'MPIX_Get_accumulate_local_atomic', 'MPIX_Get_accumulate_local_atomic_async',
           'MPIX_Compare_and_swap_local_atomic', 'MPIX_Compare_and_swap_local_atomic_async',
           'MPIX_Accumulate_atomic_is_supported']
OPS = [H.MPI_MAX, H.MPI_MIN, H.MPI_SUM, H.MPI_PROD, H.MPI_LAND, H.MPI_BAND, H.MPI_LOR, H.MPI_BOR,
       H.MPI_LXOR, H.MPI_BXOR, H.MPI_MINLOC, H.MPI_MAXLOC, H.MPI_REPLACE, H.MPI_NO_OP]
TYPES = sorted({v for k, v in vars(H).items()
                if k.startswith(('MPI_', 'MPIX_', 'MPIR_')) and isinstance(v, int)
                and (v >> 24) in (0x4c, 0x8c)})
INT_RAW = [H.MPIR_INT8, H.MPIR_INT16, H.MPIR_INT32, H.MPIR_INT64, H.MPIR_UINT8, H.MPIR_UINT16,
           H.MPIR_UINT32, H.MPIR_UINT64]


def acc(origin, target, count, dt=H.MPI_FLOAT, op=H.MPI_SUM):
    """the async and the sync entry must give the same class"""
    args = (origin, target, count, H.as_c_int(dt), H.as_c_int(op))
    rc = R.lib().MPIX_Accumulate_local_atomic_async(*args, None)
    assert R.lib().MPIX_Redop_last_error() == rc
    assert R.lib().MPIX_Accumulate_local_atomic(*args) == rc
    return rc


def ga(origin, result, target, count, dt=H.MPI_FLOAT, op=H.MPI_SUM):
    args = (origin, result, target, count, H.as_c_int(dt), H.as_c_int(op))
    rc = R.lib().MPIX_Get_accumulate_local_atomic_async(*args, None)
    assert R.lib().MPIX_Redop_last_error() == rc
    assert R.lib().MPIX_Get_accumulate_local_atomic(*args) == rc
    return rc


def both(origin, result, target, count, dt=H.MPI_FLOAT, op=H.MPI_SUM):
    """one class from the fetch and the non-fetch form"""
    rc = ga(origin, result, target, count, dt, op)
    assert acc(origin, target, count, dt, op) == rc
    return rc


def cas(origin, compare, result, target, dt=H.MPI_INT):
    args = (origin, compare, result, target, H.as_c_int(dt))
    rc = R.lib().MPIX_Compare_and_swap_local_atomic_async(*args, None)
    assert R.lib().MPIX_Redop_last_error() == rc
    assert R.lib().MPIX_Compare_and_swap_local_atomic(*args) == rc
    return rc


# ------------------------------------------------------------ the symbols
def test_header_library_and_mirror_have_the_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'mpix_redop.h')).read()
    exported = subprocess.run(['nm', '-D', '--defined-only', LIB], capture_output=True, text=True,
                              check=True).stdout
    for name in ENTRIES:
        assert re.search(r'\bint %s\(' % name, hdr), name
        assert re.search(r' T %s$' % name, exported, re.M), name
        assert getattr(R.lib(), name).argtypes is not None
    for name in ('accumulate_local_atomic', 'get_accumulate_local_atomic',
                 'compare_and_swap_local_atomic', 'accumulate_atomic_is_supported'):
        assert callable(getattr(R, name))
        assert getattr(mpich_amd, name) is getattr(R, name)
    # the header says what the step is not atomic against
    assert 'NOT atomic against' in hdr and 'NOT across devices' in hdr


# ---------------------------------------------------------- the predicate
def test_predicate_is_legal_and_kernel_and_extent():
    """legal (the oracle's MPIR_Internal_op_dt_check), a kernel in the existing
    table (the library declines bf16 other than SUM, nothing else), extent 1, 2,
    4 or 8 (the oracle's extent of the internal type)"""
    assert len(TYPES) > 60
    yes = 0
    seen_ext = set()
    for dt in TYPES:
        it = orc.internal(dt)
        ext = orc.extent(dt)
        for op in OPS:
            legal = bool(orc.internal_op_dt_check(op, it)) and ext > 0
            kernel = not ((it & 0xffffff00) == H.MPIR_BFLOAT16
                          and op not in (H.MPI_SUM, H.MPI_REPLACE, H.MPI_NO_OP))
            want = legal and kernel and ext in (1, 2, 4, 8)
            assert R.accumulate_atomic_is_supported(op, dt) == want, (hex(dt), hex(op))
            if legal and kernel:
                assert R.has_gpu_path(op, dt)
                seen_ext.add(ext)
            yes += want
        assert not R.accumulate_atomic_is_supported(H.MPIX_EQUAL, dt)
        want = (it & 0xffffff00) in INT_RAW
        assert R.accumulate_atomic_is_supported(H.MPI_OP_NULL, dt) == want, hex(dt)
    assert yes > 300
    assert seen_ext == {1, 2, 4, 8, 16, 32}
    for op in (0, 0x58000000, 0x58000010, 0x18000001, -1):
        assert not R.lib().MPIX_Accumulate_atomic_is_supported(op, H.as_c_int(H.MPI_INT))
    for dt in (0, 0x0c000000, 0x4c0000ff, -1):
        assert not R.lib().MPIX_Accumulate_atomic_is_supported(H.as_c_int(H.MPI_SUM), dt)


def test_declined_pairs_by_name():
    for dt, op in ((H.MPIR_INT128, H.MPI_SUM), (H.MPI_DOUBLE_INT, H.MPI_MAXLOC),
                   (H.MPI_LONG_INT, H.MPI_MINLOC), (H.MPI_LONG_DOUBLE_INT, H.MPI_MAXLOC),
                   (H.MPI_C_DOUBLE_COMPLEX, H.MPI_SUM), (H.MPI_LONG_DOUBLE, H.MPI_MAX),
                   (H.MPI_DOUBLE_INT, H.MPI_REPLACE), (H.MPI_LONG_DOUBLE, H.MPI_NO_OP),
                   (H.MPIX_BFLOAT16, H.MPI_MAX)):
        assert R.has_gpu_path(op, dt) == (dt != H.MPIX_BFLOAT16)
        assert not R.accumulate_atomic_is_supported(op, dt), (hex(dt), hex(op))
    for dt, op in ((H.MPI_SHORT_INT, H.MPI_MAXLOC), (H.MPI_FLOAT_INT, H.MPI_MINLOC),
                   (H.MPI_2INT, H.MPI_MAXLOC), (H.MPI_C_FLOAT_COMPLEX, H.MPI_PROD),
                   (H.MPIX_BFLOAT16, H.MPI_SUM), (H.MPI_LOGICAL, H.MPI_LXOR),
                   (H.MPI_INT8_T, H.MPI_PROD), (H.MPI_SHORT_INT, H.MPI_REPLACE)):
        assert R.accumulate_atomic_is_supported(op, dt), (hex(dt), hex(op))


def test_every_pair_agrees_with_the_entries():
    """with valid arguments and wild pointers a supported pair gets as far as
    the placement check (MPI_ERR_BUFFER), a declined legal one is MPI_ERR_TYPE"""
    for dt in TYPES:
        if R.datatype_extent(dt) <= 0:
            continue
        for op in OPS:
            if not R.internal_op_dt_check(op, R.datatype_internal(dt)):
                continue
            want = H.MPI_ERR_BUFFER if R.accumulate_atomic_is_supported(op, dt) else H.MPI_ERR_TYPE
            assert both(A, B, C, 1, dt, op) == want, (hex(dt), hex(op))


# ------------------------------------------------ errors, in their order
def test_errors_in_getacc_validates_order():
    # count < 0 first
    assert both(None, None, None, -1, 0x4c0000ff, H.MPIX_EQUAL) == H.MPI_ERR_COUNT
    # MPIX_EQUAL before the type and before count == 0
    assert both(A, B, C, 16, H.MPI_BYTE, H.MPIX_EQUAL) == H.MPI_ERR_OP
    assert both(A, B, C, 0, 0x4c0000ff, H.MPIX_EQUAL) == H.MPI_ERR_OP
    # a non-builtin op, an unknown type, an illegal pair
    assert both(A, B, C, 4, H.MPI_FLOAT, H.MPI_OP_NULL) == H.MPI_ERR_OP
    assert both(A, B, C, 4, 0x4c0000ff, H.MPI_OP_NULL) == H.MPI_ERR_OP
    assert both(A, B, C, 4, 0x4c0000ff, H.MPI_SUM) == H.MPI_ERR_TYPE
    assert both(A, B, C, 4, H.MPI_FLOAT, H.MPI_BAND) == H.MPI_ERR_OP
    assert both(A, B, C, 4, H.MPI_FLOAT, H.MPI_MAXLOC) == H.MPI_ERR_OP
    # count == 0 succeeds without looking at a pointer, a declined pair included
    for op in (H.MPI_SUM, H.MPI_NO_OP, H.MPI_REPLACE):
        assert both(None, WILD, None, 0, H.MPI_FLOAT, op) == H.MPI_SUCCESS
    assert both(WILD, None, WILD, 0, H.MPI_DOUBLE_INT, H.MPI_MAXLOC) == H.MPI_SUCCESS
    # the 2^56 cap before the pointers
    assert both(None, None, None, ((1 << 56) // 4) + 1) == H.MPI_ERR_COUNT
    assert both(None, None, None, ((1 << 56) // 16) + 1, H.MPI_DOUBLE_INT, H.MPI_MAXLOC) \
        == H.MPI_ERR_COUNT
    # NULL / MPI_IN_PLACE before the declined pair
    for bad in (None, WILD):
        assert both(bad, B, C, 4, H.MPI_DOUBLE_INT, H.MPI_MAXLOC) == H.MPI_ERR_BUFFER
        assert both(A, B, bad, 4, H.MPI_DOUBLE_INT, H.MPI_MAXLOC) == H.MPI_ERR_BUFFER
        assert ga(A, bad, C, 4, H.MPI_DOUBLE_INT, H.MPI_MAXLOC) == H.MPI_ERR_BUFFER
        assert acc(A, C, 4, H.MPI_DOUBLE_INT, H.MPI_MAXLOC) == H.MPI_ERR_TYPE   # no result to miss
    # MPI_NO_OP does not read the origin, and only MPI_NO_OP
    assert both(None, B, C, 4, H.MPIR_INT128, H.MPI_NO_OP) == H.MPI_ERR_TYPE
    assert both(None, B, C, 4, H.MPIR_INT128, H.MPI_REPLACE) == H.MPI_ERR_BUFFER
    # pairwise overlap before the declined pair
    n, ext = 4, 16
    last = (n - 1) * ext
    assert both(A, B, A + last, n, H.MPI_DOUBLE_INT, H.MPI_MAXLOC) == H.MPI_ERR_BUFFER
    assert ga(A, A + last, C, n, H.MPI_DOUBLE_INT, H.MPI_MAXLOC) == H.MPI_ERR_BUFFER
    assert ga(A, B, B + last, n, H.MPI_DOUBLE_INT, H.MPI_MAXLOC) == H.MPI_ERR_BUFFER
    assert ga(C, B, B + last, n, H.MPI_DOUBLE_INT, H.MPI_NO_OP) == H.MPI_ERR_BUFFER
    assert acc(B, B + last, n, H.MPI_DOUBLE_INT, H.MPI_NO_OP) == H.MPI_ERR_TYPE  # origin ignored
    # a declined pair before the alignment
    assert both(A, B, C + 4, 4, H.MPI_DOUBLE_INT, H.MPI_MAXLOC) == H.MPI_ERR_TYPE
    assert both(A, B, C, 4, H.MPIX_BFLOAT16, H.MPI_MAX) == H.MPI_ERR_TYPE
    assert both(A, B, C, 4, H.MPI_C_DOUBLE_COMPLEX, H.MPI_SUM) == H.MPI_ERR_TYPE
    assert both(A, B, C, 4, H.MPI_LONG_DOUBLE, H.MPI_SUM) == H.MPI_ERR_TYPE


def test_misaligned_target():
    """MPI_ERR_BUFFER is also where an aligned wild target ends (no device
    here); the order against MPI_ERR_TYPE above pins where the check stands,
    the distinguishing cases run on the GPU (tests/test_acc_atomic_gpu.py)"""
    for dt, off in ((H.MPI_FLOAT, 2), (H.MPI_INT, 1), (H.MPI_DOUBLE, 4), (H.MPI_INT64_T, 4),
                    (H.MPI_FLOAT_INT, 4), (H.MPI_SHORT_INT, 4), (H.MPI_C_FLOAT_COMPLEX, 4),
                    (H.MPI_INT16_T, 1)):
        assert both(A, B, C + off, 4, dt, H.MPI_SUM if dt not in (H.MPI_FLOAT_INT, H.MPI_SHORT_INT)
                    else H.MPI_MAXLOC) == H.MPI_ERR_BUFFER
    # origin and result need the element's alignment only in the kernels
    assert both(A + 1, B + 3, C + 1, 4, H.MPI_INT8_T, H.MPI_SUM) == H.MPI_ERR_BUFFER


def test_compare_and_swap_checks():
    for dt in TYPES:
        raw = R.datatype_internal(dt) & 0xffffff00
        if raw in INT_RAW:
            want = H.MPI_ERR_BUFFER
        else:       # the 16-byte integers included
            want = H.MPI_ERR_TYPE
        assert cas(A, B, C, D, dt) == want, hex(dt)
        if raw not in INT_RAW + [H.MPIR_INT128, H.MPIR_UINT128]:
            assert cas(None, None, None, None, dt) == H.MPI_ERR_TYPE, hex(dt)
    # MPIX_Compare_and_swap_local's checks come first for the 16-byte types
    for dt in (H.MPIR_INT128, H.MPIR_UINT128):
        assert cas(None, B, C, D, dt) == H.MPI_ERR_BUFFER
        assert cas(A, B, C, C + 15, dt) == H.MPI_ERR_BUFFER
        assert cas(A, B, C, D + 8, dt) == H.MPI_ERR_TYPE
    for bad in (None, WILD):
        for k in range(4):
            args = [A, B, C, D]
            args[k] = bad
            assert cas(*args) == H.MPI_ERR_BUFFER
    assert cas(A, B, A + 3, D) == H.MPI_ERR_BUFFER
    for dt, off in ((H.MPI_INT, 2), (H.MPI_INT64_T, 4), (H.MPI_INT16_T, 1)):
        assert cas(A, B, C, D + off, dt) == H.MPI_ERR_BUFFER


def test_python_mirror_checks_every_operand():
    big, other, third = (np.zeros(16, np.float32) for _ in range(3))
    short = np.zeros(15, np.float32)
    for bufs in ((short, big, other), (big, short, other), (big, other, short)):
        with pytest.raises(ValueError):
            R.get_accumulate_local_atomic(*bufs, 16, H.MPI_FLOAT, H.MPI_SUM, stream=0)
    for bufs in ((short, big), (big, short)):
        with pytest.raises(ValueError):
            R.accumulate_local_atomic(*bufs, 16, H.MPI_FLOAT, H.MPI_SUM, stream=0)
    with pytest.raises(ValueError):
        R.get_accumulate_local_atomic(None, short, big, 16, H.MPI_FLOAT, H.MPI_NO_OP, sync=True)
    ok = [np.zeros(1, np.int64) for _ in range(4)]
    for k in range(4):
        bufs = list(ok)
        bufs[k] = np.zeros(1, np.int32)
        with pytest.raises(ValueError):
            R.compare_and_swap_local_atomic(*bufs, H.MPI_INT64_T, stream=0)
    # in bounds: the C call refuses the pageable operands
    assert R.get_accumulate_local_atomic(big, other, third, 16, H.MPI_FLOAT, H.MPI_SUM,
                                         stream=0) == H.MPI_ERR_BUFFER
    assert R.accumulate_local_atomic(big, other, 16, H.MPI_FLOAT, H.MPI_SUM, sync=True) \
        == H.MPI_ERR_BUFFER
    assert R.compare_and_swap_local_atomic(*ok, H.MPI_INT64_T, stream=0) == H.MPI_ERR_BUFFER


# ------------------------------------------------------------ no HIP call
def test_predicate_and_argument_errors_make_no_hip_call(shim):  # noqa: F811
    calls = '\n'.join([
        'INT8, INT16, DOUBLE, DOUBLE_INT, INT128 = 0x4c000137, 0x4c000238, 0x4c00080b,'
        ' 0x8c000001, 0x4c811000',
        'EQUAL, NO_OP, OP_NULL, BAND = 0x5800000f, 0x5800000e, 0x18000000, 0x58000006',
        'P = L.MPIX_Accumulate_atomic_is_supported',
        'assert P(SUM, FLOAT) == 1 and P(SUM, INT8) == 1 and P(MAXLOC, TWOINT) == 1',
        'assert P(MAXLOC, DOUBLE_INT) == 0 and P(SUM, INT128) == 0 and P(EQUAL, INT8) == 0',
        'assert P(OP_NULL, INT16) == 1 and P(OP_NULL, FLOAT) == 0 and P(OP_NULL, INT128) == 0',
        'A_, B_, C_, D_ = 0x100000, 0x200000, 0x300000, 0x400000',
        'acc = [L.MPIX_Accumulate_local_atomic_async, L.MPIX_Accumulate_local_atomic]',
        'acc[0].argtypes = [vp, vp, a, i, i, vp]; acc[1].argtypes = [vp, vp, a, i, i]',
        'ga = [L.MPIX_Get_accumulate_local_atomic_async, L.MPIX_Get_accumulate_local_atomic]',
        'ga[0].argtypes = [vp, vp, vp, a, i, i, vp]; ga[1].argtypes = [vp, vp, vp, a, i, i]',
        'cs = [L.MPIX_Compare_and_swap_local_atomic_async, L.MPIX_Compare_and_swap_local_atomic]',
        'cs[0].argtypes = [vp, vp, vp, vp, i, vp]; cs[1].argtypes = [vp, vp, vp, vp, i]',
        'def both(want, o, r, t, n, dt, op):',
        '    assert acc[0](o, t, n, dt, op, None) == want, (want, 0)',
        '    assert acc[1](o, t, n, dt, op) == want, (want, 1)',
        '    assert ga[0](o, r, t, n, dt, op, None) == want, (want, 2)',
        '    assert ga[1](o, r, t, n, dt, op) == want, (want, 3)',
        'both(2, A_, B_, C_, -1, FLOAT, SUM)                 # MPI_ERR_COUNT',
        'both(9, A_, B_, C_, 4, INT8, EQUAL)                 # MPI_ERR_OP',
        'both(9, A_, B_, C_, 4, FLOAT, BAND)',
        'both(3, A_, B_, C_, 4, 0x4c0000ff, SUM)             # MPI_ERR_TYPE',
        'both(0, None, None, None, 0, FLOAT, SUM)            # nothing to do',
        'both(2, A_, B_, C_, (1 << 54) + 1, FLOAT, SUM)      # the cap',
        'both(1, A_, B_, None, 4, FLOAT, SUM)                # MPI_ERR_BUFFER: NULL',
        'both(1, A_, A_ + 12, A_ + 15, 4, FLOAT, SUM)        # overlap',
        'both(3, A_, B_, C_, 4, DOUBLE_INT, MAXLOC)          # declined',
        'both(3, A_, B_, C_, 4, INT128, SUM)',
        'both(1, A_, B_, C_ + 2, 4, FLOAT, SUM)              # misaligned target',
        'both(1, A_, B_, C_ + 4, 4, DOUBLE, SUM)',
        'for f in cs:',
        '    tail = (None,) if f is cs[0] else ()',
        '    assert f(A_, B_, C_, D_, FLOAT, *tail) == 3',
        '    assert f(A_, B_, C_, D_, INT128, *tail) == 3',
        '    assert f(A_, B_, None, D_, INT16, *tail) == 1',
        '    assert f(A_, B_, C_, C_ + 1, INT16, *tail) == 1',
        '    assert f(A_, B_, C_, D_ + 1, INT16, *tail) == 1',
    ])
    hits, last = _probe(shim, calls)
    assert hits == 0, 'HIP entered through %s' % last


def test_positive_control_placement_check_is_intercepted(shim):  # noqa: F811
    """an accepted call does reach the runtime (the placement check)"""
    calls = '\n'.join([
        'f = L.MPIX_Accumulate_local_atomic_async',
        'f.argtypes = [vp, vp, a, i, i, vp]',
        'assert f(0x100000, 0x200000, 4, FLOAT, SUM, None) != 0',
    ])
    hits, last = _probe(shim, calls)
    assert hits > 0 and last.startswith('hip'), (hits, last)


# ---------------------------------------------------- the built code objects
@pytest.fixture(scope='module')
def kernels():
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip('ROCm llvm tools not found')
    objs = sorted(glob.glob(os.path.join(BUILD, 'inst_acc_atomic_*.o')))
    if not objs:
        pytest.skip('library objects not built (run __graft_entry__.build())')
    return {os.path.basename(o): _kernels(o) for o in objs}


WORD, SUB, CAS = '_ZN4mpix12k_acc_atomicI', '_ZN4mpix16k_acc_atomic_subI', '_ZN4mpix12k_cas_atomicI'


def test_units_hold_the_atomic_kernels_only(kernels):
    assert sorted(kernels) == ['inst_acc_atomic_%s.o' % u for u in ('copy', 'fp', 'int', 'pair')]
    for u in ('int', 'fp', 'pair'):
        names = [k[0] for k in kernels['inst_acc_atomic_%s.o' % u]]
        assert names and all(n.startswith((WORD, SUB)) for n in names), \
            [n for n in names if not n.startswith((WORD, SUB))][:3]
        assert len(names) % 2 == 0          # a fetch and a non-fetch kernel per combiner
    names = [k[0] for k in kernels['inst_acc_atomic_copy.o']]
    assert sum(n.startswith(CAS) for n in names) == 4
    assert all(n.startswith((WORD, SUB, CAS)) for n in names)
    # no kernel for a unit wider than 8 bytes: the 16-byte integers, the x87 /
    # binary128 types and double complex are the entries' null launchers
    every = [n for ks in kernels.values() for n, _, _, _ in ks]
    assert not [n for n in every if re.search(r'I[no]E|X87|Quad|CplxIdE|DoubleIntBody|LongIntBody', n)]


def test_kernels_have_a_zero_private_segment(kernels):
    every = [k for ks in kernels.values() for k in ks]
    assert len(every) > 150
    assert not [(n, p) for n, _, p, _ in every if p][:5]
    assert not [n for n, _, _, k in every if k < 0][:5]     # no hidden arguments either
