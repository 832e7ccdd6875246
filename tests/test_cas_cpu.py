"""MPIX_Compare_and_swap_local[_async]: every refusal decided before any
device work, on a machine without a GPU, and the Python mirror's bounds.

Wild pointers stand for buffers: a refused call never looks at them."""
import ctypes

import numpy as np
import pytest

from mpich_amd import handles as H
from mpich_amd import redop as R

O, C, Z, T = 0x100000, 0x200000, 0x300000, 0x400000     # never dereferenced
WILD = ctypes.c_void_p(-1).value

INTERNAL = [H.MPIR_INT8, H.MPIR_INT16, H.MPIR_INT32, H.MPIR_INT64, H.MPIR_INT128,
            H.MPIR_UINT8, H.MPIR_UINT16, H.MPIR_UINT32, H.MPIR_UINT64, H.MPIR_UINT128]


def cas(origin, compare, result, target, dt=H.MPI_INT):
    """the async and the sync entry must give the same class"""
    args = (origin, compare, result, target, H.as_c_int(dt))
    rc = R.lib().MPIX_Compare_and_swap_local_async(*args, None)
    assert R.lib().MPIX_Redop_last_error() == rc
    assert R.lib().MPIX_Compare_and_swap_local(*args) == rc
    return rc


def test_legal_types_are_the_integer_group():
    """MPIR_Type_is_rma_atomic (rmatypeutil.c:18-30): a legal type gets as far
    as the placement check, anything else is MPI_ERR_TYPE whatever the buffers"""
    types = sorted({v for k, v in vars(H).items()
                    if k.startswith(('MPI_', 'MPIX_', 'MPIR_')) and isinstance(v, int)
                    and (v >> 24) in (0x4c, 0x8c)})
    assert len(types) > 60
    legal = 0
    for dt in types:
        raw = R.datatype_internal(dt) & 0xffffff00
        want = H.MPI_ERR_BUFFER if raw in INTERNAL else H.MPI_ERR_TYPE
        assert cas(O, C, Z, T, dt) == want, hex(dt)
        if want == H.MPI_ERR_TYPE:
            assert cas(None, None, None, None, dt) == H.MPI_ERR_TYPE, hex(dt)
        legal += want == H.MPI_ERR_BUFFER
    assert legal >= 20
    for dt in INTERNAL + [H.MPI_INT, H.MPI_LONG, H.MPI_UNSIGNED_CHAR, H.MPI_INT64_T, H.MPI_AINT]:
        assert cas(O, C, Z, T, dt) == H.MPI_ERR_BUFFER, hex(dt)
    for dt in (H.MPI_FLOAT, H.MPI_DOUBLE, H.MPI_DOUBLE_INT, H.MPI_2INT, H.MPI_LOGICAL,
               H.MPI_LOGICAL4, H.MPI_C_DOUBLE_COMPLEX, H.MPIX_BFLOAT16, H.MPI_LONG_DOUBLE,
               0x4c0000ff, 0x0c000000):
        assert cas(O, C, Z, T, dt) == H.MPI_ERR_TYPE, hex(dt)


def test_null_buffers():
    for bad in (None, WILD):
        for k in range(4):
            args = [O, C, Z, T]
            args[k] = bad
            assert cas(*args) == H.MPI_ERR_BUFFER


@pytest.mark.parametrize('dt,size', [(H.MPI_INT8_T, 1), (H.MPI_INT, 4), (H.MPIR_UINT128, 16)])
def test_overlaps(dt, size):
    """MPI_ERR_BUFFER is also where a disjoint wild quadruple ends, so the
    overlap arithmetic is pinned through the sync form's order: it refuses a
    non-device target only after the overlap check, with the same class; the
    distinguishing cases run on the GPU (tests/test_cas_gpu.py)"""
    last = size - 1
    for z in (O, O + last, O - last, C, C + last, T, T - last):
        assert cas(O, C, z, T, dt) == H.MPI_ERR_BUFFER
    for t in (O, O + last, C, C - last):
        assert cas(O, C, Z, t, dt) == H.MPI_ERR_BUFFER
    assert cas(O, O, Z, T, dt) == H.MPI_ERR_BUFFER      # allowed: the placement check refuses


def test_python_mirror_checks_every_operand():
    ok = [np.zeros(1, np.int64) for _ in range(4)]
    for k in range(4):
        bufs = list(ok)
        bufs[k] = np.zeros(1, np.int32)
        with pytest.raises(ValueError):
            R.compare_and_swap_local(*bufs, H.MPI_INT64_T, stream=0)
        with pytest.raises(ValueError):
            R.compare_and_swap_local(*bufs, H.MPI_INT64_T, sync=True)
    # in bounds: the C call refuses the pageable operands
    assert R.compare_and_swap_local(*ok, H.MPI_INT64_T, stream=0) == H.MPI_ERR_BUFFER
    assert R.compare_and_swap_local(*ok, H.MPI_INT64_T, sync=True) == H.MPI_ERR_BUFFER
