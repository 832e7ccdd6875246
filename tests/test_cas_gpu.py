"""MPIX_Compare_and_swap_local[_async] on the GPU: result = the target's value,
target = origin exactly where compare == target as integers of the element's
size (posix_rma.h:605-608), the bytes around all four operands untouched."""
import numpy as np
import pytest
import torch

from tests.test_getacc_gpu import Placed

pytestmark = pytest.mark.gpu


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


TYPES = [('MPIR_INT8', 1), ('MPIR_INT16', 2), ('MPIR_INT32', 4), ('MPIR_INT64', 8),
         ('MPIR_INT128', 16), ('MPIR_UINT8', 1), ('MPIR_UINT16', 2), ('MPIR_UINT32', 4),
         ('MPIR_UINT64', 8), ('MPIR_UINT128', 16),
         ('MPI_INT', 4), ('MPI_LONG', 8), ('MPI_UNSIGNED_CHAR', 1), ('MPI_SHORT', 2),
         ('MPI_UINT64_T', 8), ('MPI_INTEGER16', 16), ('MPI_AINT', 8), ('MPI_BYTE', 1)]


def one(R, dt, origin, compare, target, offs=(0, 0, 0, 0), sync=False, same=False):
    """one call on placed operands; returns (result bytes, target bytes) after
    checking the origin, the compare operand and every guard byte.  same: the
    compare operand IS the origin's address"""
    size = len(target)
    O, C, T = Placed(origin, offs[0]), Placed(compare, offs[1]), Placed(target, offs[3])
    Z = Placed(np.full(size, 0xA5, np.uint8), offs[2])
    torch.cuda.synchronize()
    assert R.compare_and_swap_local(O.v, O.v if same else C.v, Z.v, T.v, dt, sync=sync) == 0
    if not sync:
        torch.cuda.synchronize()
    assert np.array_equal(O.bytes(), origin) and np.array_equal(C.bytes(), compare)
    assert O.guards_intact() and C.guards_intact() and Z.guards_intact() and T.guards_intact()
    return Z.bytes(), T.bytes()


@pytest.mark.parametrize('name,size', TYPES, ids=[t[0] for t in TYPES])
def test_types_and_values(R, H, name, size):
    dt = getattr(H, name)
    assert R.datatype_extent(dt) == size
    rng = np.random.default_rng(0x5EED0D00 + size + len(name))
    for rep in range(2):
        target = rng.integers(0, 256, size, dtype=np.uint8)
        origin = rng.integers(0, 256, size, dtype=np.uint8)
        origin[0] = target[0] ^ 0x3c                         # never equal to the target
        offs = (0, 0, 0, 0) if rep == 0 else (size, 2 * size, 3 * size, size)
        msb, lsb, other = target.copy(), target.copy(), target.copy()
        msb[-1] ^= 0x80                                      # little endian: the top bit
        lsb[0] ^= 0x01
        other[:] = rng.integers(0, 256, size, dtype=np.uint8)
        other[size // 2] = target[size // 2] ^ 0xff
        for compare, swaps in ((target.copy(), True), (other, False), (msb, False), (lsb, False)):
            z, t = one(R, dt, origin, compare, target, offs)
            assert np.array_equal(z, target), 'result is the old target'
            assert np.array_equal(t, origin if swaps else target), (name, swaps)


def test_off_the_element_grid(R, H):
    """no operand needs any alignment (as the contiguous fetch entry at count 1)"""
    rng = np.random.default_rng(0x5EED0D10)
    for name, size in (('MPI_INT', 4), ('MPI_INT64_T', 8), ('MPIR_UINT128', 16)):
        target = rng.integers(0, 256, size, dtype=np.uint8)
        origin = target ^ 0x55
        for offs in ((1, 0, 0, 0), (0, 3, 0, 0), (0, 0, 5, 0), (0, 0, 0, 7), (1, 2, 3, 5)):
            z, t = one(R, getattr(H, name), origin, target.copy(), target, offs)
            assert np.array_equal(z, target) and np.array_equal(t, origin)


def test_origin_and_compare_at_the_same_address(R, H):
    rng = np.random.default_rng(0x5EED0D20)
    v = rng.integers(0, 256, 8, dtype=np.uint8)
    z, t = one(R, H.MPI_INT64_T, v, v, v.copy(), same=True)     # equal: swapped for the same value
    assert np.array_equal(z, v) and np.array_equal(t, v)
    w = v ^ 0x10
    z, t = one(R, H.MPI_INT64_T, v, v, w, same=True)            # different: left alone
    assert np.array_equal(z, w) and np.array_equal(t, w)


def test_chained_counter_on_one_stream(R, H):
    """100 calls without synchronising, compare = i and origin = i + 1; call 50
    carries a stale compare, so the counter stops there: every later compare
    is one ahead of the target"""
    n, stale = 100, 50
    cmp_ = np.arange(n, dtype=np.int64)
    cmp_[stale] = stale - 7
    C, O = Placed(cmp_), Placed(np.arange(1, n + 1, dtype=np.int64))
    Z, T = Placed(np.full(8 * n, 0xA5, np.uint8)), Placed(np.zeros(1, np.int64))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for i in range(n):
        sl = slice(8 * i, 8 * i + 8)
        assert R.compare_and_swap_local(O.v[sl], C.v[sl], Z.v[sl], T.v, H.MPI_INT64_T,
                                        stream=s) == 0
    s.synchronize()
    want = np.where(np.arange(n) <= stale, np.arange(n), stale)
    assert np.array_equal(Z.bytes().view(np.int64), want)
    assert T.bytes().view(np.int64)[0] == stale
    assert Z.guards_intact() and T.guards_intact() and C.guards_intact() and O.guards_intact()


def test_sync_form(R, H):
    """returns with result and target visible: read back on another stream"""
    rng = np.random.default_rng(0x5EED0D30)
    for name, size in (('MPI_INT', 4), ('MPIR_UINT128', 16)):
        target = rng.integers(0, 256, size, dtype=np.uint8)
        origin = target ^ 0x0f
        z, t = one(R, getattr(H, name), origin, target.copy(), target, sync=True)
        assert np.array_equal(z, target) and np.array_equal(t, origin)
        z, t = one(R, getattr(H, name), origin, origin.copy(), target, sync=True)
        assert np.array_equal(z, target) and np.array_equal(t, target)
    P = [Placed(np.zeros(4, np.uint8)) for _ in range(4)]
    host = np.zeros(1, np.int32)
    torch.cuda.synchronize()
    # sync: a device-memory target; async: no pageable operand at all
    assert R.compare_and_swap_local(P[0].v, P[1].v, P[2].v, host, H.MPI_INT,
                                    sync=True) == H.MPI_ERR_BUFFER
    for k in range(4):
        bufs = [p.v for p in P]
        bufs[k] = host
        assert R.compare_and_swap_local(*bufs, H.MPI_INT) == H.MPI_ERR_BUFFER
    torch.cuda.synchronize()
    assert all(not p.bytes().any() and p.guards_intact() for p in P)


def quad(size, seed):
    rng = np.random.default_rng(seed)
    raw = [rng.integers(0, 256, 64, dtype=np.uint8) for _ in range(4)]
    raw[1][:size] = raw[3][:size]           # compare == target: a run call would swap
    return raw, [Placed(x) for x in raw]


def unchanged(raw, P):
    torch.cuda.synchronize()
    return all(np.array_equal(p.bytes(), x) and p.guards_intact() for p, x in zip(P, raw))


@pytest.mark.parametrize('name', ['MPI_FLOAT', 'MPI_DOUBLE_INT', 'MPI_LOGICAL', 'MPI_DOUBLE',
                                  'MPI_2INT', 'MPI_C_FLOAT_COMPLEX'])
def test_refused_types_touch_nothing(R, H, name):
    raw, P = quad(16, 0x5EED0D40)
    for sync in (False, True):
        assert R.compare_and_swap_local(P[0].v, P[1].v, P[2].v, P[3].v, getattr(H, name),
                                        sync=sync) == H.MPI_ERR_TYPE
    assert unchanged(raw, P)


@pytest.mark.parametrize('name,size', [('MPI_INT8_T', 1), ('MPI_INT', 4), ('MPIR_INT128', 16)])
def test_overlaps(R, H, name, size):
    """every refused overlap, by one byte and whole, is MPI_ERR_BUFFER with
    nothing touched; operands that only touch are served"""
    dt = getattr(H, name)
    raw, P = quad(size, 0x5EED0D50 + size)
    o, c, z, t = (p.v for p in P)
    last = size - 1
    refused = [(o, c, o, t), (o, c, o[last:], t), (o[last:], c, o, t),       # result / origin
               (o, c, c, t), (o, c, c[last:], t),                           # result / compare
               (o, c, t, t), (o, c, t[last:], t), (o, c, z, z[last:]),      # result / target
               (t, c, z, t), (t[last:], c, z, t),                           # target / origin
               (o, t, z, t), (o, c, z, c[last:])]                           # target / compare
    for sync in (False, True):
        for args in refused:
            assert R.compare_and_swap_local(*args, dt, sync=sync) == H.MPI_ERR_BUFFER
    assert unchanged(raw, P)
    # touching operands, origin and compare sharing bytes: served
    x = Placed(np.concatenate([raw[3][:size]] * 4))          # [origin = compare | result | target]
    torch.cuda.synchronize()
    assert R.compare_and_swap_local(x.v, x.v, x.v[size:], x.v[2 * size:], dt) == 0
    torch.cuda.synchronize()
    assert np.array_equal(x.bytes(), np.concatenate([raw[3][:size]] * 4)) and x.guards_intact()
