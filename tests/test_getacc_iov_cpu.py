"""The fetch entries over iov / iovec targets
(MPIX_Get_accumulate_local_iov_async, MPIX_Get_accumulate_local_iovec_async):
every error class decided before any device work, on a machine without a GPU,
the Python mirror's range checks, and what the new instantiation units hold,
read from the built code objects.

Wild pointers stand for buffers: a call that is refused, or that has nothing
to do, never looks at them."""
import ctypes
import os

import numpy as np
import pytest

from mpich_amd import handles as H
from mpich_amd import redop as R
from tests.test_kernel_resources import BUILD, OBJDUMP, READELF, _kernels

A, B, C = 0x100000, 0x200000, 0x300000      # three disjoint "buffers", never dereferenced
WILD = ctypes.c_void_p(-1).value
AINT = ctypes.c_ssize_t


def tab(xs):
    return (AINT * max(len(xs), 1))(*xs)


def gi(origin, result, target, offs, cnts, dt=H.MPI_DOUBLE, op=H.MPI_SUM, nseg=None):
    rc = R.lib().MPIX_Get_accumulate_local_iov_async(
        origin, result, target, len(offs) if nseg is None else nseg, tab(offs), tab(cnts),
        H.as_c_int(dt), H.as_c_int(op), None)
    assert R.lib().MPIX_Redop_last_error() == rc
    return rc


def gv(origin, result, target, offs, lens, dt=H.MPI_DOUBLE, op=H.MPI_SUM, nseg=None):
    rc = R.lib().MPIX_Get_accumulate_local_iovec_async(
        origin, result, target, len(offs) if nseg is None else nseg, tab(offs), tab(lens),
        H.as_c_int(dt), H.as_c_int(op), None)
    assert R.lib().MPIX_Redop_last_error() == rc
    return rc


def both(origin, result, target, offs, cnts, dt=H.MPI_DOUBLE, op=H.MPI_SUM):
    """the iov form and the iovec form of the same runs of a basic type"""
    size = R.datatype_size(dt)
    rc = gi(origin, result, target, offs, cnts, dt, op)
    assert gv(origin, result, target, offs, [c * size for c in cnts], dt, op) == rc
    return rc


def test_table_errors_come_first():
    assert gi(A, B, C, [0], [1], nseg=-1) == H.MPI_ERR_COUNT
    assert gv(A, B, C, [0], [8], nseg=-1) == H.MPI_ERR_COUNT
    lib = R.lib()
    for f in (lib.MPIX_Get_accumulate_local_iov_async, lib.MPIX_Get_accumulate_local_iovec_async):
        assert f(A, B, C, 1, None, tab([1]), H.as_c_int(H.MPI_DOUBLE), H.as_c_int(H.MPI_SUM),
                 None) == H.MPI_ERR_BUFFER
        assert f(A, B, C, 1, tab([0]), None, H.as_c_int(H.MPI_DOUBLE), H.as_c_int(H.MPI_SUM),
                 None) == H.MPI_ERR_BUFFER
        # ... before the type, the op and the buffers
        assert f(None, None, None, -1, None, None, 0x4c0000ff, 0x18000000, None) == H.MPI_ERR_COUNT
    assert gi(A, B, C, [0, 64], [2, -1]) == H.MPI_ERR_COUNT
    assert gv(A, B, C, [0, 64], [16, -8]) == H.MPI_ERR_COUNT
    # a negative count before the type and the op
    assert gi(None, None, None, [0], [-1], 0x4c0000ff, H.MPI_BAND) == H.MPI_ERR_COUNT


def test_type_then_op_then_buffers():
    assert both(A, B, C, [0], [1], 0x4c0000ff, H.MPI_SUM) == H.MPI_ERR_TYPE     # unknown type
    assert gi(None, None, None, [2], [1], 0x4c0000ff, H.MPI_BAND) == H.MPI_ERR_TYPE
    assert both(A, B, C, [0], [1], H.MPI_DOUBLE, H.MPI_BAND) == H.MPI_ERR_OP    # illegal pair
    assert both(A, B, C, [0], [1], H.MPI_DOUBLE, H.MPI_MAXLOC) == H.MPI_ERR_OP
    assert both(A, B, C, [0], [1], H.MPI_DOUBLE, 0x18000000) == H.MPI_ERR_OP    # MPI_OP_NULL
    # an illegal pair before NULL buffers and before a misaligned residue
    assert gi(None, None, None, [2], [1], H.MPI_DOUBLE, H.MPI_LXOR) == H.MPI_ERR_OP
    # NULL buffers before the residue, the residue before the overlap
    assert gi(A, None, C, [2], [1]) == H.MPI_ERR_BUFFER
    assert gi(A, A, A, [2], [1]) == H.MPI_ERR_ARG


def test_equal_is_refused():
    assert both(A, B, C, [0], [16], H.MPI_BYTE, H.MPIX_EQUAL) == H.MPI_ERR_OP
    assert both(A, B, C, [], [], H.MPI_BYTE, H.MPIX_EQUAL) == H.MPI_ERR_OP


def test_declined_pair_is_a_type_error():
    assert R.internal_op_dt_check(H.MPI_MAX, H.MPIR_BFLOAT16)
    assert both(A, B, C, [0], [4], H.MPIX_BFLOAT16, H.MPI_MAX) == H.MPI_ERR_TYPE
    assert both(A, B, C, [0], [4], H.MPIX_BFLOAT16, H.MPI_PROD) == H.MPI_ERR_TYPE


def test_every_pair_with_a_fetch_kernel_has_a_fetch_iov_kernel():
    """with valid arguments and wild pointers a pair the contiguous fetch entry
    covers gets as far as the placement check (MPI_ERR_BUFFER) here too, an
    uncovered one is MPI_ERR_TYPE in both"""
    types = sorted({v for k, v in vars(H).items()
                    if k.startswith(('MPI_', 'MPIX_', 'MPIR_')) and isinstance(v, int)
                    and (v >> 24) in (0x4c, 0x8c)})
    ops = [H.MPI_MAX, H.MPI_MIN, H.MPI_SUM, H.MPI_PROD, H.MPI_LAND, H.MPI_BAND, H.MPI_LOR,
           H.MPI_BOR, H.MPI_LXOR, H.MPI_BXOR, H.MPI_MINLOC, H.MPI_MAXLOC]
    assert len(types) > 60
    covered = 0
    for dt in types:
        for op in ops:
            if not (R.internal_op_dt_check(op, R.datatype_internal(dt))
                    and R.datatype_extent(dt) > 0):
                continue
            contig = R.lib().MPIX_Get_accumulate_local_async(A, B, C, 1, H.as_c_int(dt),
                                                             H.as_c_int(op), None)
            assert contig in (H.MPI_ERR_BUFFER, H.MPI_ERR_TYPE)
            assert gi(A, B, C, [0], [1], dt, op) == contig, (hex(dt), hex(op))
            assert (contig == H.MPI_ERR_BUFFER) == R.has_gpu_path(op, dt)
            covered += contig == H.MPI_ERR_BUFFER
    assert covered > 300


def test_null_buffers():
    for bad in (None, WILD):
        assert both(bad, B, C, [0], [4]) == H.MPI_ERR_BUFFER
        assert both(A, bad, C, [0], [4]) == H.MPI_ERR_BUFFER
        assert both(A, B, bad, [0], [4]) == H.MPI_ERR_BUFFER
    # MPI_NO_OP does not read the origin: NULL passes the checks (the call then
    # fails on the wild result / target pointers, not on the origin)
    assert both(None, None, C, [0], [4], H.MPI_DOUBLE, H.MPI_NO_OP) == H.MPI_ERR_BUFFER
    assert both(None, B, None, [0], [4], H.MPI_DOUBLE, H.MPI_NO_OP) == H.MPI_ERR_BUFFER
    assert both(None, B, C, [0], [4], H.MPI_DOUBLE, H.MPI_REPLACE) == H.MPI_ERR_BUFFER


def test_zero_total_touches_no_pointer():
    for op in (H.MPI_SUM, H.MPI_NO_OP, H.MPI_REPLACE):
        assert both(None, WILD, None, [], [], H.MPI_DOUBLE, op) == H.MPI_SUCCESS
        assert both(WILD, None, WILD, [0, 64, -8], [0, 0, 0], H.MPI_DOUBLE, op) == H.MPI_SUCCESS
        # not even the residue of a run that covers nothing
        assert gi(WILD, None, WILD, [3], [0], H.MPI_DOUBLE, op) == H.MPI_SUCCESS
    # a padded pair's segments that never complete an element
    assert gv(WILD, None, WILD, [0], [8], H.MPI_DOUBLE_INT, H.MPI_MAXLOC) == H.MPI_SUCCESS


def test_misaligned_residue():
    assert gi(A, B, C, [0, 66], [2, 2]) == H.MPI_ERR_ARG                    # 2 mod 8
    assert gi(A, B, C, [0, 68], [2, 2]) == H.MPI_ERR_BUFFER                 # 4 mod 8 is fine
    assert gi(A, B, C, [-10], [2]) == H.MPI_ERR_ARG
    assert gi(A, B, C, [1], [2], H.MPI_INT16_T, H.MPI_SUM) == H.MPI_ERR_ARG
    assert gi(A, B, C, [2], [2], H.MPI_INT16_T, H.MPI_SUM) == H.MPI_ERR_BUFFER
    assert gi(A, B, C, [3], [2], H.MPI_INT8_T, H.MPI_SUM) == H.MPI_ERR_BUFFER


def test_iovec_partial_element():
    assert gv(A, B, C, [0], [12]) == H.MPI_ERR_ARG
    assert gv(A, B, C, [0, 64], [16, 4]) == H.MPI_ERR_ARG
    # decided while the iov is read: before the op and the buffers
    assert gv(None, None, None, [0], [12], H.MPI_DOUBLE, H.MPI_BAND) == H.MPI_ERR_ARG
    # MPI_FLOAT_INT has no padding: a 4-byte segment is a partial element
    assert gv(A, B, C, [0, 4], [4, 4], H.MPI_FLOAT_INT, H.MPI_MAXLOC) == H.MPI_ERR_ARG
    assert gv(A, B, C, [0], [8], H.MPI_FLOAT_INT, H.MPI_MAXLOC) == H.MPI_ERR_BUFFER
    # a padded pair gathers {value, int}
    assert gv(A, B, C, [0, 8], [8, 4], H.MPI_DOUBLE_INT, H.MPI_MAXLOC) == H.MPI_ERR_BUFFER


def test_span_cap():
    top = 1 << 56
    assert gi(A, B, C, [0], [top // 8]) == H.MPI_ERR_COUNT                  # packed range
    assert gi(A, B, C, [0], [top // 8 - 1]) == H.MPI_ERR_BUFFER             # under the cap: overlap
    assert gi(A, B, C, [0, 0], [top // 16, top // 16]) == H.MPI_ERR_COUNT   # the sum
    assert gi(A, B, C, [0, top - 8], [1, 1]) == H.MPI_ERR_COUNT             # bounding range
    assert gi(A, B, C, [-(top // 2), top // 2 - 8], [1, 1]) == H.MPI_ERR_COUNT
    assert gi(A, B, C, [-(1 << 62), (1 << 62)], [1, 1]) == H.MPI_ERR_COUNT
    assert gi(A, B, C, [0, (1 << 62)], [1, 0]) == H.MPI_ERR_BUFFER          # an empty run: no bound
    assert gv(A, B, C, [0], [top]) == H.MPI_ERR_COUNT
    assert gi(A, B, C, [0], [(1 << 63) - 1]) == H.MPI_ERR_COUNT


def test_bounding_range_overlaps():
    """two fp64 runs of 4 elements at bytes -64 and +96 of the target pointer:
    bounding range [T - 64, T + 128), packed operands 64 bytes"""
    offs, cnts, T = [96, -64], [4, 4], B
    assert gi(A, C, T, offs, cnts) == H.MPI_ERR_BUFFER        # disjoint: the placement check
    for z in (T - 64, T - 32, T + 32, T + 127, T - 127):      # runs and the gap between alike
        assert gi(A, z, T, offs, cnts) == H.MPI_ERR_BUFFER
        assert gi(z, C, T, offs, cnts) == H.MPI_ERR_BUFFER
    # just outside on either side: no overlap, so the refusal is the placement
    # check's, which MPI_NO_OP with a NULL origin reaches as well
    for z in (T - 128, T + 128):
        assert gi(None, z, T, offs, cnts, H.MPI_DOUBLE, H.MPI_NO_OP) == H.MPI_ERR_BUFFER
    assert gi(A, A + 63, T, offs, cnts) == H.MPI_ERR_BUFFER     # origin / result
    # MPI_NO_OP ignores the origin altogether
    assert gi(T, C, T, offs, cnts, H.MPI_DOUBLE, H.MPI_NO_OP) == H.MPI_ERR_BUFFER


def test_overlap_is_told_from_placement():
    """MPI_ERR_BUFFER is also what a wild but disjoint triple ends in, so pin
    the overlap arithmetic where the two differ: a legal pair without a kernel
    is MPI_ERR_TYPE only once the overlap check has passed"""
    offs, cnts, T = [96, -64], [4, 4], B
    dt, op = H.MPIX_BFLOAT16, H.MPI_MAX         # packed 16 bytes, range [T - 64, T + 104)
    assert gi(A, C, T, offs, cnts, dt, op) == H.MPI_ERR_TYPE
    for z in (T - 80, T + 104):                 # touching, not overlapping
        assert gi(A, z, T, offs, cnts, dt, op) == H.MPI_ERR_TYPE
        assert gi(z, C, T, offs, cnts, dt, op) == H.MPI_ERR_TYPE
    for z in (T - 79, T - 64, T, T + 50, T + 103):
        assert gi(A, z, T, offs, cnts, dt, op) == H.MPI_ERR_BUFFER
        assert gi(z, C, T, offs, cnts, dt, op) == H.MPI_ERR_BUFFER
    assert gi(A, A + 15, T, offs, cnts, dt, op) == H.MPI_ERR_BUFFER
    assert gi(A, A + 16, T, offs, cnts, dt, op) == H.MPI_ERR_TYPE


def test_python_mirror_checks_every_operand():
    offs, cnts = [16, 64], [2, 3]               # fp64: target bytes [16, 88), packed 40
    tgt, pk = np.zeros(11, np.float64), np.zeros(5, np.float64)
    short = np.zeros(4, np.float64)
    args = (offs, cnts, H.MPI_DOUBLE, H.MPI_SUM)
    for bufs in ((short, pk, tgt), (pk, short, tgt), (pk, pk.copy(), np.zeros(10, np.float64))):
        with pytest.raises(ValueError):
            R.get_accumulate_local_iov(*bufs, *args, stream=0)
    with pytest.raises(ValueError):             # origin=None: the other two are still checked
        R.get_accumulate_local_iov(None, short, tgt, offs, cnts, H.MPI_DOUBLE, H.MPI_NO_OP,
                                   stream=0)
    with pytest.raises(ValueError):             # the lowest run byte lies before the buffer
        R.get_accumulate_local_iov(pk, pk.copy(), tgt, [-8, 64], cnts, H.MPI_DOUBLE, H.MPI_SUM,
                                   stream=0)
    lens = [16, 24]
    for bufs in ((short, pk, tgt), (pk, short, tgt), (pk, pk.copy(), np.zeros(10, np.float64))):
        with pytest.raises(ValueError):
            R.get_accumulate_local_iovec(*bufs, offs, lens, H.MPI_DOUBLE, H.MPI_SUM, stream=0)
    with pytest.raises(ValueError):
        R.get_accumulate_local_iovec(pk, pk.copy(), tgt[1:], [-16, 64], lens, H.MPI_DOUBLE,
                                     H.MPI_SUM, stream=0)
    # a negative offset inside the storage of a view passes the mirror; the C
    # call then refuses the pageable operands
    assert R.get_accumulate_local_iov(pk, pk.copy(), tgt[2:], [-16, 48], cnts, H.MPI_DOUBLE,
                                      H.MPI_SUM, stream=0) == H.MPI_ERR_BUFFER


# ---------------------------------------------------- the built code objects
UNITS = ['inst_getacc_iov_%s.o' % u for u in ('int', 'fp', 'pair')] + ['inst_getacc_copy.o']
FETCH, COPY, CAS = '_ZN4mpix12k_getacc_iovI', '_ZN4mpix17k_getacc_iov_copyI', '_ZN4mpix5k_casI'


@pytest.fixture(scope='module')
def kernels():
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip('ROCm llvm tools not found')
    objs = [os.path.join(BUILD, u) for u in UNITS]
    if not all(os.path.exists(o) for o in objs):
        pytest.skip('library objects not built (run __graft_entry__.build())')
    return {u: _kernels(o) for u, o in zip(UNITS, objs)}


def test_new_units_hold_only_the_new_kernel_families(kernels):
    """one fetch-iov kernel per combiner of the contiguous fetch units, the
    copy kernel per unit body and mode, compare-and-swap per element size"""
    fetch = [k[0] for u in UNITS[:3] for k in kernels[u]]
    assert all(n.startswith(FETCH) for n in fetch), \
        [n for n in fetch if not n.startswith(FETCH)][:3]
    elem = 0
    for u in ('int', 'fp', 'pair'):
        elem += sum(k[0].startswith('_ZN4mpix13k_getacc_elemI')
                    for k in _kernels(os.path.join(BUILD, 'inst_getacc_%s.o' % u)))
    assert len(fetch) == elem >= 100
    other = [k[0] for k in kernels[UNITS[3]]]
    assert all(n.startswith((COPY, CAS)) for n in other), other
    assert sum(n.startswith(COPY) for n in other) == 2 * 9      # 6 raw units, 3 padded pairs
    assert sum(n.startswith(CAS) for n in other) == 5


def test_new_kernels_use_no_scratch_and_no_hidden_arguments(kernels):
    ks = [k for u in UNITS for k in kernels[u]]
    assert not [(n, p) for n, _, p, _ in ks if p][:5]
    assert not [n for n, _, _, k in ks if k < 0][:5]
