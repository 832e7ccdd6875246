"""The fused get-accumulate entries (MPIX_Get_accumulate_local*): every error
class decided before any device work, on a machine without a GPU, the Python
mirror's span check, and the register / argument budget of the new kernels
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

A, B, C = 0x10000, 0x20000, 0x30000     # three disjoint "buffers", never dereferenced
ASYNC = None


def ga(origin, result, target, count, dt=H.MPI_FLOAT, op=H.MPI_SUM):
    """the async and the sync entry must give the same class"""
    args = (origin, result, target, count, H.as_c_int(dt), H.as_c_int(op))
    rc = R.lib().MPIX_Get_accumulate_local_async(*args, ASYNC)
    assert R.lib().MPIX_Get_accumulate_local(*args) == rc
    assert R.lib().MPIX_Redop_last_error() == rc
    return rc


def gav(origin, result, target, count, bl, st, dt=H.MPI_DOUBLE, op=H.MPI_SUM):
    args = (origin, result, target, count, bl, st, H.as_c_int(dt), H.as_c_int(op))
    rc = R.lib().MPIX_Get_accumulate_local_vector_async(*args, ASYNC)
    assert R.lib().MPIX_Get_accumulate_local_vector(*args) == rc
    return rc


def test_negative_count():
    assert ga(A, B, C, -1) == H.MPI_ERR_COUNT
    assert gav(A, B, C, -1, 1, 2) == H.MPI_ERR_COUNT
    assert gav(A, B, C, 4, -1, 2) == H.MPI_ERR_COUNT


def test_op_and_type_legality():
    assert ga(A, B, C, 4, H.MPI_FLOAT, H.MPI_BAND) == H.MPI_ERR_OP       # illegal pair
    assert ga(A, B, C, 4, H.MPI_FLOAT, H.MPI_MAXLOC) == H.MPI_ERR_OP
    assert ga(A, B, C, 4, H.MPI_FLOAT, 0x18000000) == H.MPI_ERR_OP       # MPI_OP_NULL
    assert ga(A, B, C, 4, 0x4c0000ff, H.MPI_SUM) == H.MPI_ERR_TYPE       # unknown type
    assert gav(A, B, C, 4, 1, 2, H.MPI_DOUBLE, H.MPI_LXOR) == H.MPI_ERR_OP


def test_equal_is_refused():
    assert ga(A, B, C, 16, H.MPI_BYTE, H.MPIX_EQUAL) == H.MPI_ERR_OP
    assert ga(A, B, C, 0, H.MPI_BYTE, H.MPIX_EQUAL) == H.MPI_ERR_OP
    assert gav(A, B, C, 16, 1, 2, H.MPI_BYTE, H.MPIX_EQUAL) == H.MPI_ERR_OP


def test_declined_pair_is_a_type_error():
    """a legal pair without a kernel, refused before any buffer is looked at"""
    assert R.internal_op_dt_check(H.MPI_MAX, H.MPIR_BFLOAT16)
    assert not R.has_gpu_path(H.MPI_MAX, H.MPIX_BFLOAT16)
    assert ga(A, B, C, 4, H.MPIX_BFLOAT16, H.MPI_MAX) == H.MPI_ERR_TYPE
    assert gav(A, B, C, 4, 1, 2, H.MPIX_BFLOAT16, H.MPI_PROD) == H.MPI_ERR_TYPE


def test_every_pair_with_a_reduce_kernel_has_a_fetch_kernel():
    """has_gpu_path answers for these entries as for MPIX_Reduce_local: with
    valid arguments and wild pointers a covered pair gets as far as the
    placement check (MPI_ERR_BUFFER), an uncovered one is MPI_ERR_TYPE"""
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
            rc = R.lib().MPIX_Get_accumulate_local_async(A, B, C, 1, H.as_c_int(dt),
                                                         H.as_c_int(op), ASYNC)
            want = H.MPI_ERR_BUFFER if R.has_gpu_path(op, dt) else H.MPI_ERR_TYPE
            assert rc == want, (hex(dt), hex(op), rc)
            covered += rc == H.MPI_ERR_BUFFER
    assert covered > 300


def test_null_buffers():
    for bad in (None, ctypes.c_void_p(-1).value):
        assert ga(bad, B, C, 4) == H.MPI_ERR_BUFFER
        assert ga(A, bad, C, 4) == H.MPI_ERR_BUFFER
        assert ga(A, B, bad, 4) == H.MPI_ERR_BUFFER
        assert gav(bad, B, C, 4, 1, 2) == H.MPI_ERR_BUFFER
        assert gav(A, bad, C, 4, 1, 2) == H.MPI_ERR_BUFFER
        assert gav(A, B, bad, 4, 1, 2) == H.MPI_ERR_BUFFER
    # MPI_NO_OP does not read the origin: NULL passes the checks (the call
    # then fails on the wild result / target pointers, not on the origin)
    assert ga(None, None, C, 4, H.MPI_FLOAT, H.MPI_NO_OP) == H.MPI_ERR_BUFFER
    assert ga(None, B, None, 4, H.MPI_FLOAT, H.MPI_NO_OP) == H.MPI_ERR_BUFFER
    assert ga(None, B, C, 0, H.MPI_FLOAT, H.MPI_NO_OP) == H.MPI_SUCCESS
    # ... and only for MPI_NO_OP
    assert ga(None, B, C, 4, H.MPI_FLOAT, H.MPI_REPLACE) == H.MPI_ERR_BUFFER


def test_pairwise_overlaps():
    n, ext = 16, 4
    last = (n - 1) * ext        # one element shared
    assert ga(A, B, A + last, n) == H.MPI_ERR_BUFFER        # origin / target
    assert ga(A, A + last, C, n) == H.MPI_ERR_BUFFER        # origin / result
    assert ga(A, B, B + last, n) == H.MPI_ERR_BUFFER        # result / target
    assert ga(A, B + last, B, n) == H.MPI_ERR_BUFFER
    assert ga(A, A, A, n) == H.MPI_ERR_BUFFER
    # MPI_NO_OP ignores the origin altogether, result / target still count
    assert ga(C, B, B + last, n, H.MPI_FLOAT, H.MPI_NO_OP) == H.MPI_ERR_BUFFER


def test_vector_span_overlap():
    count, bl, st, ext = 8, 2, 5, 8
    span = ((count - 1) * st + bl) * ext        # 296 bytes, the packed operands 128
    packed = count * bl * ext
    assert gav(A, B, A + packed - 1, count, bl, st) == H.MPI_ERR_BUFFER
    assert gav(A + span - 1, B, A, count, bl, st) == H.MPI_ERR_BUFFER     # inside a gap or not
    assert gav(A, B + packed, B + packed - span + 1, count, bl, st) == H.MPI_ERR_BUFFER
    assert gav(A, B + span - 1, B, count, bl, st) == H.MPI_ERR_BUFFER
    assert gav(A, B, B + packed - 1, count, bl, st) == H.MPI_ERR_BUFFER


def test_stride_below_blocklen():
    assert gav(A, B, C, 4, 3, 2) == H.MPI_ERR_ARG


def test_span_cap():
    ext = 4
    assert ga(A, B, C, ((1 << 56) // ext) + 1) == H.MPI_ERR_COUNT
    assert gav(A, B, C, (1 << 40), 1, (1 << 20), H.MPI_DOUBLE) == H.MPI_ERR_COUNT
    assert gav(A, B, C, (1 << 30), (1 << 30), (1 << 30), H.MPI_DOUBLE) == H.MPI_ERR_COUNT


def test_count_zero_touches_no_pointer():
    wild = ctypes.c_void_p(-1).value
    for op in (H.MPI_SUM, H.MPI_NO_OP, H.MPI_REPLACE):
        assert ga(None, wild, None, 0, H.MPI_FLOAT, op) == H.MPI_SUCCESS
        assert gav(wild, None, wild, 0, 3, 5, H.MPI_DOUBLE, op) == H.MPI_SUCCESS
        assert gav(wild, None, wild, 7, 0, 5, H.MPI_DOUBLE, op) == H.MPI_SUCCESS


def test_python_mirror_checks_every_operand():
    big = np.zeros(16, np.float32)
    short = np.zeros(15, np.float32)
    other = np.zeros(16, np.float32)
    for bufs in ((short, big, other), (big, short, other), (big, other, short)):
        with pytest.raises(ValueError):
            R.get_accumulate_local(*bufs, 16, H.MPI_FLOAT, H.MPI_SUM, stream=0)
    with pytest.raises(ValueError):     # origin=None: the other two are still checked
        R.get_accumulate_local(None, short, big, 16, H.MPI_FLOAT, H.MPI_NO_OP, stream=0)
    tgt = np.zeros(2 * 7 + 1, np.float64)           # span of (8, 1, 2) is 15 elements
    pk = np.zeros(8, np.float64)
    with pytest.raises(ValueError):
        R.get_accumulate_local_vector(pk, pk.copy(), np.zeros(14, np.float64), 8, 1, 2,
                                      H.MPI_DOUBLE, H.MPI_SUM, stream=0)
    with pytest.raises(ValueError):
        R.get_accumulate_local_vector(pk, pk[:7].copy(), tgt, 8, 1, 2, H.MPI_DOUBLE, H.MPI_SUM,
                                      stream=0)
    with pytest.raises(ValueError):
        R.get_accumulate_local_vector(pk[:7].copy(), pk, tgt, 8, 1, 2, H.MPI_DOUBLE, H.MPI_SUM,
                                      stream=0)


# ---------------------------------------------------- the built code objects
@pytest.fixture(scope='module')
def kernels():
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip('ROCm llvm tools not found')
    objs = [os.path.join(BUILD, 'inst_getacc_%s.o' % u) for u in ('int', 'fp', 'pair')]
    if not all(os.path.exists(o) for o in objs):
        pytest.skip('library objects not built (run __graft_entry__.build())')
    ks = []
    for o in objs:
        ks += _kernels(o)
    return ks


PACKET, ELEM, VECTOR = '_ZN4mpix8k_getaccI', '_ZN4mpix13k_getacc_elemI', '_ZN4mpix15k_getacc_vectorI'


def test_new_kernels_are_the_get_accumulate_ones(kernels):
    """the units hold nothing else, two packet variants at most per combiner
    and one element-wise and one vector kernel for every combiner"""
    names = [k[0] for k in kernels]
    assert all(n.startswith((PACKET, ELEM, VECTOR)) for n in names), \
        [n for n in names if not n.startswith((PACKET, ELEM, VECTOR))][:3]
    ne = sum(n.startswith(ELEM) for n in names)
    assert ne >= 100
    assert sum(n.startswith(VECTOR) for n in names) == ne
    assert 0 < sum(n.startswith(PACKET) for n in names) <= 2 * ne


def test_new_kernels_use_no_scratch_and_no_hidden_arguments(kernels):
    assert not [(n, p) for n, _, p, _ in kernels if p][:5]
    assert not [n for n, _, _, k in kernels if k < 0][:5]


def test_packet_kernels_under_the_vgpr_cap(kernels):
    packet = [(n, v) for n, v, _, _ in kernels if n.startswith(PACKET)]
    worst = max(packet, key=lambda x: x[1])
    assert worst[1] <= 96, worst
