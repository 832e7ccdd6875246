"""The fused get-accumulate (MPIX_Get_accumulate_local*) on the GPU.

Every case checks four things:
  * `result` holds the target's bytes from before the call, bit for bit (the
    padded pairs: the data fields, the result's own padding untouched);
  * `target` equals oracle.reduce_local(origin, target_before) under the
    parity rule of tests/test_gpu_parity.py (compare);
  * `target` is bit-identical to what MPIX_Reduce_local_async leaves on a copy
    of the same operands at the same alignment;
  * `origin`, and the guard bytes around all three operands, are unchanged.
"""
import threading

import numpy as np
import pytest
import torch

from tests import test_soft_fp as S
from tests.test_gpu_parity import SWEEP, compare, make_operand
from tests.test_ldouble_gpu import loc_records

pytestmark = pytest.mark.gpu

GUARD, CANARY = 0x5A, 0xA5
SLACK = 64


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


class Placed:
    """`data` at byte offset `off` from a 256-byte-aligned device address,
    guard bytes on both sides"""

    def __init__(self, data, off=0, device='cuda'):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.nb = len(data)
        self.buf = torch.full((self.nb + 512 + 2 * SLACK,), GUARD, dtype=torch.uint8, device=device)
        self.lo = (-self.buf.data_ptr()) % 256 + SLACK + off
        self.v = self.buf[self.lo:self.lo + self.nb]
        self.v.copy_(torch.from_numpy(data.copy()))
        assert (self.v.data_ptr() - off - SLACK) % 256 == 0

    def bytes(self):
        return self.v.cpu().numpy()

    def guards_intact(self):
        h = self.buf.cpu().numpy()
        return bool((h[:self.lo] == GUARD).all() and (h[self.lo + self.nb:] == GUARD).all())


def field_mask(H, dt, ext):
    """bytes of one element that belong to its type map"""
    m = np.ones(ext, bool)
    if dt in (H.MPI_DOUBLE_INT, H.MPI_LONG_INT):
        m[12:] = False
    elif dt == H.MPI_SHORT_INT:
        m[2:4] = False
    elif dt == H.MPI_LONG_DOUBLE_INT:
        m[20:] = False
    return m


def expected_result(H, dt, ext, target_before, n):
    exp = np.full((n, ext), CANARY, np.uint8)
    m = field_mask(H, dt, ext)
    exp[:, m] = target_before.reshape(n, ext)[:, m]
    return exp.reshape(-1)


def fetch_and_check(R, H, oracle, dt, op, n, tgt, org, offs=(0, 0, 0), parity=None, call=None):
    """one get-accumulate of `n` elements against the four expectations;
    offs = byte offsets of (target, origin, result); parity = (kind, size,
    opname) for the oracle comparison; call(O, Z, T) replaces the default
    stream-ordered call.  Returns the target's bytes after the call."""
    ext = R.datatype_extent(dt)
    tgt = np.ascontiguousarray(tgt).view(np.uint8).reshape(-1)
    org = np.ascontiguousarray(org).view(np.uint8).reshape(-1)
    assert len(tgt) == n * ext and len(org) == n * ext
    T, O = Placed(tgt, offs[0]), Placed(org, offs[1])
    Z = Placed(np.full(n * ext, CANARY, np.uint8), offs[2])
    T2, O2 = Placed(tgt, offs[0]), Placed(org, offs[1])
    torch.cuda.synchronize()
    if call is None:
        assert R.get_accumulate_local(O.v, Z.v, T.v, n, dt, op) == 0
    else:
        call(O, Z, T)
    assert R.reduce_local_async(O2.v, T2.v, n, dt, op) == 0
    torch.cuda.synchronize()
    got = T.bytes()
    assert np.array_equal(Z.bytes(), expected_result(H, dt, ext, tgt, n)), 'result'
    assert np.array_equal(O.bytes(), org), 'origin changed'
    assert np.array_equal(got, T2.bytes()), 'target differs from MPIX_Reduce_local_async'
    assert T.guards_intact() and O.guards_intact() and Z.guards_intact(), 'guard bytes'
    if parity:
        kind, size, opname = parity
        exp = tgt.copy()
        assert oracle.reduce_local(org.copy(), exp, n, dt, op) == 0
        assert compare(got, exp, kind, size, opname, ext) == 0
    return got


# 1 ------------------------------------------- packet kernel, head and tail
EDGE_TYPES = [('MPI_FLOAT', 'MPI_SUM', 'fp', 4), ('MPI_INT8_T', 'MPI_MAX', 'int', 1),
              ('MPI_INT16_T', 'MPI_BXOR', 'int', 2), ('MPI_DOUBLE', 'MPI_PROD', 'fp', 8),
              ('MPI_INTEGER16', 'MPI_SUM', 'int', 16)]
EDGE_COUNTS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4099]


@pytest.mark.parametrize('n', EDGE_COUNTS)
@pytest.mark.parametrize('dtname,opname,kind,size', EDGE_TYPES, ids=[t[0] for t in EDGE_TYPES])
def test_packet_head_and_tail_edges(R, H, oracle, dtname, opname, kind, size, n):
    """count below the head, both packet variants (origin and result on the
    target's 16-byte phase or off it by an element) and the tail"""
    dt, op = getattr(H, dtname), getattr(H, opname)
    ext = R.datatype_extent(dt)
    rng = np.random.default_rng(0x5EED0A00 + 131 * n + ext)
    tgt = make_operand(rng, kind, size, n, dtname)
    org = make_operand(rng, kind, size, n, dtname)
    toffs = [0, ext] + ([3 * ext] if 3 * ext < 16 else [])
    for toff in toffs:
        for ooff in (0, ext):
            for roff in (0, ext):
                fetch_and_check(R, H, oracle, dt, op, n, tgt, org, (toff, ooff, roff),
                                (kind, size, opname))


def test_not_element_aligned(R, H, oracle):
    """operands off the element grid go element-wise"""
    n = 4099
    rng = np.random.default_rng(0x5EED0A05)
    tgt = make_operand(rng, 'fp', 4, n, 'MPI_FLOAT')
    org = make_operand(rng, 'fp', 4, n, 'MPI_FLOAT')
    for offs in ((2, 0, 0), (0, 2, 0), (0, 0, 6), (2, 2, 2)):
        fetch_and_check(R, H, oracle, H.MPI_FLOAT, H.MPI_SUM, n, tgt, org, offs,
                        ('fp', 4, 'MPI_SUM'))


# 2 --------------------------------------------------- every pair of SWEEP
@pytest.mark.parametrize('dtname,opname,kind,size', SWEEP,
                         ids=['%s-%s' % (s[0], s[1]) for s in SWEEP])
def test_every_pair_off_phase(R, H, oracle, dtname, opname, kind, size):
    dt, op = getattr(H, dtname), getattr(H, opname)
    ext = R.datatype_extent(dt)
    n = 4099
    rng = np.random.default_rng((0x5EED0A10 * 31 + dt * 7 + op) & 0xffffffff)
    tgt = make_operand(rng, kind, size, n, dtname)
    org = make_operand(rng, kind, size, n, dtname)
    fetch_and_check(R, H, oracle, dt, op, n, tgt, org, (0, ext, ext), (kind, size, opname))


# 3 ------------------------------------- 32-byte units and split combiners
def _soft_operands(H, rng, dtname, n, zero_im):
    """operands from the soft-fp / long-double suites' generators"""
    x87 = 'LONG_DOUBLE' in dtname
    rand = (lambda: S.x87_random(rng, n, True)) if x87 else (lambda: S.quad_random(rng, n, True))
    sp = np.stack(S.x87_specials() if x87 else S.quad_specials())

    def part():
        p = rand()
        p[::9] = sp[rng.integers(0, len(sp), len(p[::9]))]
        return p
    if dtname in ('MPI_LONG_DOUBLE', 'MPI_REAL16'):
        return part(), part()
    if dtname == 'MPI_LONG_DOUBLE_INT':
        return loc_records(part(), part(), rng, 16)
    re_a, im_a, re_b, im_b = part(), part(), part(), part()
    if zero_im:         # real values stored as complex: every product leaves the fast path
        im_a[:, :10 if x87 else 16] = 0
        im_b[:, :10 if x87 else 16] = 0
    return np.concatenate([re_a, im_a], 1), np.concatenate([re_b, im_b], 1)


SOFT = [(t, o) for t in ('MPI_LONG_DOUBLE', 'MPI_REAL16')
        for o in ('MPI_MAX', 'MPI_MIN', 'MPI_SUM', 'MPI_PROD')] + \
       [(t, o) for t in ('MPI_C_LONG_DOUBLE_COMPLEX', 'MPI_COMPLEX32')
        for o in ('MPI_SUM', 'MPI_PROD')] + \
       [('MPI_LONG_DOUBLE_INT', o) for o in ('MPI_MAXLOC', 'MPI_MINLOC')]


@pytest.mark.parametrize('n', [1, 65, 1027])
@pytest.mark.parametrize('dtname,opname', SOFT, ids=['%s-%s' % s for s in SOFT])
def test_wide_units_match_the_reduce_entry(R, H, oracle, dtname, opname, n):
    dt, op = getattr(H, dtname), getattr(H, opname)
    rng = np.random.default_rng((0x5EED0A20 + dt * 3 + op + n) & 0xffffffff)
    sets = [False, True] if 'COMPLEX' in dtname else [False]
    for zero_im in sets:
        tgt, org = _soft_operands(H, rng, dtname, n, zero_im)
        for offs in ((0, 0, 0), (0, 16, 16)):
            fetch_and_check(R, H, oracle, dt, op, n, tgt, org, offs)


# 4 ------------------------------------------ many tiles, the looping grid
def test_many_tiles(R, H, oracle):
    n = (1 << 20) + 13
    rng = np.random.default_rng(0x5EED0A30)
    tgt = make_operand(rng, 'fp', 4, n, 'MPI_FLOAT')
    org = make_operand(rng, 'fp', 4, n, 'MPI_FLOAT')
    fetch_and_check(R, H, oracle, H.MPI_FLOAT, H.MPI_SUM, n, tgt, org, (4, 0, 8),
                    ('fp', 4, 'MPI_SUM'))


def test_looping_grid(R, H, oracle):
    n = 65536 + 5
    rng = np.random.default_rng(0x5EED0A31)
    tgt = make_operand(rng, 'fp', 4, n, 'MPI_FLOAT')
    org = make_operand(rng, 'fp', 4, n, 'MPI_FLOAT')
    before = R.get_launch()
    assert R.set_launch(64, 2) == 0
    try:
        for offs in ((0, 0, 0), (4, 8, 0)):
            fetch_and_check(R, H, oracle, H.MPI_FLOAT, H.MPI_SUM, n, tgt, org, offs,
                            ('fp', 4, 'MPI_SUM'))
    finally:
        assert R.set_launch(before['block'], before['max_grid']) == 0
    assert R.get_launch() == before


# 5, 6 --------------------------------------------------- NO_OP and REPLACE
@pytest.mark.parametrize('dtname,kind,size', [('MPI_FLOAT', 'fp', 4),
                                              ('MPI_DOUBLE_INT', ('pair', '<f8', '<i4', 16, 8), None)])
def test_no_op_fetches_only(R, H, dtname, kind, size):
    dt = getattr(H, dtname)
    ext = R.datatype_extent(dt)
    n = 1027
    rng = np.random.default_rng(0x5EED0A40 + ext)
    tgt = make_operand(rng, kind, size, n, dtname)
    T = Placed(tgt, ext)
    Z = Placed(np.full(n * ext, CANARY, np.uint8), 0)
    torch.cuda.synchronize()
    assert R.get_accumulate_local(None, Z.v, T.v, n, dt, H.MPI_NO_OP) == 0
    torch.cuda.synchronize()
    assert np.array_equal(T.bytes(), tgt)
    assert np.array_equal(Z.bytes(), expected_result(H, dt, ext, tgt, n))
    assert T.guards_intact() and Z.guards_intact()


@pytest.mark.parametrize('dtname,kind,size', [('MPI_FLOAT', 'fp', 4),
                                              ('MPI_DOUBLE_INT', ('pair', '<f8', '<i4', 16, 8), None)])
def test_replace_swaps(R, H, oracle, dtname, kind, size):
    """result = old target, target = origin; a padded pair keeps the padding
    of both (fetch_and_check compares the target with the reduce entry's
    MPI_REPLACE, which keeps it)"""
    dt = getattr(H, dtname)
    ext = R.datatype_extent(dt)
    n = 1027
    rng = np.random.default_rng(0x5EED0A50 + ext)
    tgt = make_operand(rng, kind, size, n, dtname)
    org = make_operand(rng, kind, size, n, dtname)
    got = fetch_and_check(R, H, oracle, dt, H.MPI_REPLACE, n, tgt, org, (0, ext, 0))
    m = field_mask(H, dt, ext)
    exp = tgt.reshape(n, ext).copy()
    exp[:, m] = org.reshape(n, ext)[:, m]
    assert np.array_equal(got.reshape(n, ext), exp)


# 7 ------------------------------------------------------- vector target
VEC_TYPES = [('MPI_DOUBLE', 'MPI_SUM', 'fp', 8), ('MPI_DOUBLE_INT', 'MPI_MAXLOC',
                                                 ('pair', '<f8', '<i4', 16, 8), None),
             ('MPI_INT8_T', 'MPI_BOR', 'int', 1)]


@pytest.mark.parametrize('blocklen,stride', [(1, 2), (1, 3), (3, 5), (4, 4)])
@pytest.mark.parametrize('dtname,opname,kind,size', VEC_TYPES, ids=[t[0] for t in VEC_TYPES])
def test_vector_target(R, H, oracle, dtname, opname, kind, size, blocklen, stride):
    dt, op = getattr(H, dtname), getattr(H, opname)
    ext = R.datatype_extent(dt)
    count = 1031
    n = count * blocklen
    span = (count - 1) * stride + blocklen
    rng = np.random.default_rng(0x5EED0A60 + 17 * blocklen + stride + ext)
    packed_t = make_operand(rng, kind, size, n, dtname).reshape(count, blocklen * ext)
    org = make_operand(rng, kind, size, n, dtname)
    rows = np.full((count, stride * ext), CANARY, np.uint8)     # gaps hold the canary
    rows[:, :blocklen * ext] = packed_t
    tgt = rows.reshape(-1)[:span * ext].copy()
    T, O, Z = Placed(tgt), Placed(org), Placed(np.full(n * ext, CANARY, np.uint8))
    T2, O2 = Placed(tgt), Placed(org)
    torch.cuda.synchronize()
    assert R.get_accumulate_local_vector(O.v, Z.v, T.v, count, blocklen, stride, dt, op) == 0
    assert R.reduce_local_vector(O2.v, T2.v, count, blocklen, stride, dt, op) == 0
    torch.cuda.synchronize()
    got = T.bytes()
    assert np.array_equal(Z.bytes(), expected_result(H, dt, ext, packed_t.reshape(-1), n))
    assert np.array_equal(O.bytes(), org)
    assert np.array_equal(got, T2.bytes())
    assert T.guards_intact() and O.guards_intact() and Z.guards_intact()
    full = np.full(count * stride * ext, CANARY, np.uint8)
    full[:span * ext] = got
    full = full.reshape(count, stride * ext)
    assert (full[:, blocklen * ext:] == CANARY).all(), 'a gap element was written'
    exp = packed_t.reshape(-1).copy()
    assert oracle.reduce_local(org.copy(), exp, n, dt, op) == 0
    assert compare(np.ascontiguousarray(full[:, :blocklen * ext]).reshape(-1), exp, kind, size,
                   opname, ext) == 0


# 8 ---------------------------------------------------------- stream order
def test_three_chained_calls_on_one_stream(R, H):
    n = 70001
    rng = np.random.default_rng(0x5EED0A70)
    t0, o1, o2, o3 = (rng.integers(-1 << 20, 1 << 20, n).astype(np.int32) for _ in range(4))
    T = Placed(t0)
    Os = [Placed(o) for o in (o1, o2, o3)]
    Zs = [Placed(np.full(4 * n, CANARY, np.uint8)) for _ in range(3)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for O, Z in zip(Os, Zs):        # no host synchronisation in between
        assert R.get_accumulate_local(O.v, Z.v, T.v, n, H.MPI_INT, H.MPI_SUM, stream=s) == 0
    s.synchronize()
    want = [t0, t0 + o1, t0 + o1 + o2]
    for Z, w in zip(Zs, want):
        assert np.array_equal(Z.bytes().view(np.int32), w)
    assert np.array_equal(T.bytes().view(np.int32), t0 + o1 + o2 + o3)


# 9 ----------------------------------------------------------- sync forms
def test_sync_forms_return_with_the_result_visible(R, H, oracle):
    rng = np.random.default_rng(0x5EED0A80)
    for n in (1, 4099, 300000):
        tgt = make_operand(rng, 'fp', 8, n, 'MPI_DOUBLE')
        org = make_operand(rng, 'fp', 8, n, 'MPI_DOUBLE')
        seen = {}

        def call(O, Z, T):
            assert R.get_accumulate_local(O.v, Z.v, T.v, n, H.MPI_DOUBLE, H.MPI_SUM,
                                          sync=True) == 0
            # read back on another stream without any synchronisation of ours
            with torch.cuda.stream(torch.cuda.Stream()):
                seen['z'] = Z.v.to('cpu', non_blocking=False).numpy().copy()
        fetch_and_check(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, n, tgt, org, (8, 0, 8),
                        ('fp', 8, 'MPI_SUM'), call=call)
        assert np.array_equal(seen['z'], tgt)
    count, bl, st = 515, 3, 5
    n = count * bl
    tgt = rng.integers(0, 256, ((count - 1) * st + bl) * 8, dtype=np.uint8)
    org = rng.integers(0, 256, n * 8, dtype=np.uint8)
    T, O, Z = Placed(tgt), Placed(org), Placed(np.zeros(n * 8, np.uint8))
    torch.cuda.synchronize()
    assert R.get_accumulate_local_vector(O.v, Z.v, T.v, count, bl, st, H.MPI_INT64_T, H.MPI_BXOR,
                                         sync=True) == 0
    z = Z.v.cpu().numpy().view(np.uint64)
    t = np.zeros(count * st, np.uint64)
    t[:len(tgt) // 8] = tgt.view(np.uint64)
    assert np.array_equal(z, t.reshape(count, st)[:, :bl].reshape(-1))


def test_host_operands(R, H):
    n = 1000
    d = [Placed(np.zeros(4 * n, np.uint8)) for _ in range(3)]
    h = np.zeros(n, np.float32)
    torch.cuda.synchronize()
    # sync: the target must be device memory
    assert R.get_accumulate_local(d[0].v, d[1].v, h, n, H.MPI_FLOAT, H.MPI_SUM,
                                  sync=True) == H.MPI_ERR_BUFFER
    # async: no pageable operand at all
    for bufs in ((h, d[1].v, d[2].v), (d[0].v, h, d[2].v), (d[0].v, d[1].v, h)):
        assert R.get_accumulate_local(*bufs, n, H.MPI_FLOAT, H.MPI_SUM) == H.MPI_ERR_BUFFER
    torch.cuda.synchronize()
    for p in d:
        assert not p.bytes().any() and p.guards_intact()


# 10 -------------------------------------------------------- declined pair
def test_declined_pair_touches_nothing(R, H):
    n = 513
    rng = np.random.default_rng(0x5EED0A90)
    raw = [rng.integers(0, 256, 2 * n, dtype=np.uint8) for _ in range(3)]
    P = [Placed(x) for x in raw]
    torch.cuda.synchronize()
    for sync in (False, True):
        assert R.get_accumulate_local(P[0].v, P[1].v, P[2].v, n, H.MPIX_BFLOAT16, H.MPI_MAX,
                                      sync=sync) == H.MPI_ERR_TYPE
    torch.cuda.synchronize()
    for p, x in zip(P, raw):
        assert np.array_equal(p.bytes(), x) and p.guards_intact()


# 11 --------------------------------------------------------- concurrency
def test_four_threads_share_no_state(R, H, oracle):
    """each thread its own stream and buffers, the split product (whose
    reduce entry keeps per-stream fixup words) beside fp32 SUM"""
    n, rounds = 3001, 4
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            rng = np.random.default_rng(0x5EED0AA0 + k)
            s = torch.cuda.Stream()
            for r in range(rounds):
                ct, co = _soft_operands(H, rng, 'MPI_COMPLEX32', n, r % 2 == 1)
                ft = make_operand(rng, 'fp', 4, n, 'MPI_FLOAT')
                fo = make_operand(rng, 'fp', 4, n, 'MPI_FLOAT')
                want_c = ct.reshape(-1).copy()
                assert oracle.reduce_local(co.reshape(-1).copy(), want_c, n, H.MPI_COMPLEX32,
                                           H.MPI_PROD) == 0
                want_f = ft.copy()
                assert oracle.reduce_local(fo.copy(), want_f, n, H.MPI_FLOAT, H.MPI_SUM) == 0
                CT, CO, CZ = Placed(ct), Placed(co), Placed(np.zeros(32 * n, np.uint8))
                FT, FO, FZ = Placed(ft, 4), Placed(fo), Placed(np.zeros(4 * n, np.uint8), 8)
                torch.cuda.synchronize()
                assert R.get_accumulate_local(CO.v, CZ.v, CT.v, n, H.MPI_COMPLEX32, H.MPI_PROD,
                                              stream=s) == 0
                assert R.get_accumulate_local(FO.v, FZ.v, FT.v, n, H.MPI_FLOAT, H.MPI_SUM,
                                              stream=s) == 0
                s.synchronize()
                assert np.array_equal(CZ.bytes(), ct.reshape(-1))
                assert np.array_equal(CT.bytes(), want_c)
                assert np.array_equal(FZ.bytes(), ft)
                assert compare(FT.bytes(), want_f, 'fp', 4, 'MPI_SUM', 4) == 0
        except BaseException as e:      # noqa: B902 -- reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
