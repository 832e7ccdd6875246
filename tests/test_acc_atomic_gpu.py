"""The element-atomic entries (MPIX_[Get_]accumulate_local_atomic*,
MPIX_Compare_and_swap_local_atomic*) on the GPU.

  1. one caller: every supported (op, type) pair, fetch and non-fetch, sync and
     async, at every sub-dword phase of the target, leaves bit for bit the
     target and result MPIX_Get_accumulate_local_async leaves on copies, and
     the oracle's target under the parity rule of tests/test_gpu_parity.py
     (compare: the payload of an arithmetic NaN is the host's, unpinned);
  2. tickets: fetch-SUM of ones from four streams -- per element the fetched
     values are exactly 0 .. calls - 1 and the target ends at their number;
  3. swap chain: REPLACE with unique tokens from four streams;
  4. order-free folds from four streams against the oracle's fold;
  5. compare-and-swap: contended increments, parity with the non-atomic entry;
  6. two more processes on an MPIX_Ipc_open mapping of the target;
  7. refusals that need the device, every byte unchanged.

No test asserts that the non-atomic entries lose updates: they may not."""
import os
import select
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from tests.test_getacc_gpu import CANARY, GUARD, SLACK, Placed, expected_result, field_mask
from tests.test_gpu_parity import SWEEP, compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [1, 2, 3, 63, 64, 65, 257, 4099]
POOL = 4099
NTHREADS, CALLS = 4, 32


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


def extent_of(kind, size):
    if isinstance(kind, tuple):
        return kind[3]
    return 2 * size if kind == 'cplx' else size


SUPPORTED = [s for s in SWEEP if extent_of(s[2], s[3]) <= 8]
DECLINED = [s for s in SWEEP if extent_of(s[2], s[3]) > 8]


# ------------------------------------------------------------- the arena
class Arena:
    """Operands of many calls in one device allocation: each at a byte offset
    from a 256-byte-aligned address with at least SLACK guard bytes on both
    sides, uploaded once and downloaded once."""

    def __init__(self):
        self.parts = []
        self.size = 0

    def place(self, data, off):
        lo = (self.size + 255) // 256 * 256 + 256 + off
        self.parts.append((lo, np.ascontiguousarray(data).view(np.uint8).reshape(-1)))
        self.size = lo + len(self.parts[-1][1]) + SLACK
        return lo

    def upload(self):
        self.host = np.full(self.size + 256, GUARD, np.uint8)
        for lo, d in self.parts:
            self.host[lo:lo + len(d)] = d
        self.dev = torch.empty(len(self.host) + 256, dtype=torch.uint8, device='cuda')
        self.skew = (-self.dev.data_ptr()) % 256
        self.view = self.dev[self.skew:self.skew + len(self.host)]
        self.view.copy_(torch.from_numpy(self.host))
        self.base = self.view.data_ptr()
        assert self.base % 256 == 0
        torch.cuda.synchronize()

    def download(self):
        torch.cuda.synchronize()
        return self.view.cpu().numpy()


def phases(ext):
    return (0, 1, 2, 3) if ext == 1 else (0, 2) if ext == 2 else (0, ext)


def off_phase(ext, tph):
    """(origin, result) byte offsets off the target's phase"""
    mod = max(4, 2 * ext)
    o = (tph + ext) % mod
    return o, ((tph + 2 * ext) % mod if ext == 1 else o)


FORMS = [(sync, fetch) for sync in (False, True) for fetch in (True, False)]


def run_parity(R, H, oracle, dt, op, opname, kind, size, pool_t, pool_o, counts=COUNTS):
    """every (count, target phase, operand phases) case of one pair in the four
    forms, with MPIX_Get_accumulate_local_async on copies beside them"""
    ext = R.datatype_extent(dt)
    assert ext == extent_of(kind, size)
    no_op, replace = op == H.MPI_NO_OP, op == H.MPI_REPLACE
    ar = Arena()
    cases = []
    for n in counts:
        for tph in phases(ext):
            for ooff, roff in ((tph, tph), off_phase(ext, tph)):
                s = (17 * n + 5 * tph) % (POOL - n + 1)
                tgt, org = pool_t[s * ext:(s + n) * ext], pool_o[s * ext:(s + n) * ext]
                c = dict(n=n, tph=tph, tgt=tgt, org=org, o=ar.place(org, ooff),
                         t_ref=ar.place(tgt, tph),
                         z_ref=ar.place(np.full(n * ext, CANARY, np.uint8), roff), forms=[])
                for sync, fetch in FORMS:
                    t = ar.place(tgt, tph)
                    z = ar.place(np.full(n * ext, CANARY, np.uint8), roff) if fetch else None
                    c['forms'].append((sync, fetch, t, z))
                cases.append(c)
    ar.upload()
    b = ar.base
    for c in cases:                             # stream-ordered on torch's current stream
        o = None if no_op else b + c['o']
        assert R.get_accumulate_local(o, b + c['z_ref'], b + c['t_ref'], c['n'], dt, op) == 0
        for sync, fetch, t, z in c['forms']:
            if sync:
                continue
            if fetch:
                assert R.get_accumulate_local_atomic(o, b + z, b + t, c['n'], dt, op) == 0
            else:
                assert R.accumulate_local_atomic(o, b + t, c['n'], dt, op) == 0
    for c in cases:                             # the library stream; operands of their own
        o = None if no_op else b + c['o']
        for sync, fetch, t, z in c['forms']:
            if not sync:
                continue
            if fetch:
                assert R.get_accumulate_local_atomic(o, b + z, b + t, c['n'], dt, op,
                                                     sync=True) == 0
            else:
                assert R.accumulate_local_atomic(o, b + t, c['n'], dt, op, sync=True) == 0
    got = ar.download()
    exp = ar.host.copy()
    for c in cases:
        nb = c['n'] * ext
        t_ref, z_ref = got[c['t_ref']:c['t_ref'] + nb], got[c['z_ref']:c['z_ref'] + nb]
        what = (opname, c['n'], c['tph'])
        # the reference entry itself: the old target in the result's type map ...
        assert np.array_equal(z_ref, expected_result(H, dt, ext, c['tgt'], c['n'])), what
        # ... and the oracle's target
        if no_op:
            assert np.array_equal(t_ref, c['tgt']), what
        elif replace:
            m = np.tile(field_mask(H, dt, ext), c['n'])
            assert np.array_equal(t_ref, np.where(m, c['org'], c['tgt'])), what
        else:
            want = c['tgt'].copy()
            assert oracle.reduce_local(c['org'].copy(), want, c['n'], dt, op) == 0
            assert compare(t_ref, want, kind, size, opname, ext) == 0, what
        exp[c['t_ref']:c['t_ref'] + nb] = t_ref
        exp[c['z_ref']:c['z_ref'] + nb] = z_ref
        for sync, fetch, t, z in c['forms']:
            exp[t:t + nb] = t_ref
            if fetch:
                exp[z:z + nb] = z_ref
    # every form's target and result bit for bit the reference entry's, every
    # origin and every guard byte as uploaded
    if not np.array_equal(got, exp):
        at = int(np.flatnonzero(got != exp)[0])
        for c in cases:
            for sync, fetch, t, z in c['forms']:
                for name, lo in (('target', t), ('result', z)):
                    if lo is not None and lo - 256 <= at < lo + c['n'] * ext + 256:
                        pytest.fail('%s n=%d phase=%d sync=%d fetch=%d: %s byte %d is %#x, not %#x'
                                    % (opname, c['n'], c['tph'], sync, fetch, name, at - lo,
                                       got[at], exp[at]))
        pytest.fail('byte %d of the arena differs' % at)


def c3_pools(kind, size, seed):
    from bench import c3_operand
    g = torch.Generator(device='cuda')
    g.manual_seed(seed & 0xffffffff)
    t, o = c3_operand(g, kind, size, POOL), c3_operand(g, kind, size, POOL)
    torch.cuda.synchronize()
    return t.cpu().numpy(), o.cpu().numpy()


# 1 ---------------------------------------------------- one caller: parity
def test_supported_pairs_are_the_sweeps_up_to_8_bytes(R, H):
    assert len(SUPPORTED) > 120 and len(DECLINED) > 20
    for dtname, opname, _, _ in SUPPORTED:
        assert R.accumulate_atomic_is_supported(getattr(H, opname), getattr(H, dtname)), dtname
    for dtname, opname, _, _ in DECLINED:
        assert not R.accumulate_atomic_is_supported(getattr(H, opname), getattr(H, dtname)), dtname


@pytest.mark.parametrize('dtname,opname,kind,size', SUPPORTED,
                         ids=['%s-%s' % (s[0], s[1]) for s in SUPPORTED])
def test_one_caller_parity(R, H, oracle, dtname, opname, kind, size):
    dt, op = getattr(H, dtname), getattr(H, opname)
    pool_t, pool_o = c3_pools(kind, size, 0x5EED1700 * 31 + dt * 7 + op)
    run_parity(R, H, oracle, dt, op, opname, kind, size, pool_t, pool_o)


COPY_TYPES = [('MPI_INT8_T', 'int', 1), ('MPI_INT16_T', 'int', 2), ('MPI_FLOAT', 'fp', 4),
              ('MPI_DOUBLE', 'fp', 8), ('MPIR_2INT8', ('pair', '<i1', '<i1', 2, 1), None),
              ('MPI_FLOAT_INT', ('pair', '<f4', '<i4', 8, 4), None),
              ('MPI_SHORT_INT', ('pair', '<i2', '<i4', 8, 4), None)]


@pytest.mark.parametrize('opname', ['MPI_NO_OP', 'MPI_REPLACE'])
@pytest.mark.parametrize('dtname,kind,size', COPY_TYPES, ids=[t[0] for t in COPY_TYPES])
def test_no_op_and_replace_parity(R, H, oracle, dtname, kind, size, opname):
    """MPI_NO_OP with a NULL origin (an atomic fetch; nothing in the non-fetch
    form) and MPI_REPLACE (an atomic exchange / store of the type map: the
    padded pair keeps the target's padding)"""
    dt, op = getattr(H, dtname), getattr(H, opname)
    assert R.accumulate_atomic_is_supported(op, dt)
    pool_t, pool_o = c3_pools(kind, size, 0x5EED1710 * 31 + dt * 7 + op)
    run_parity(R, H, oracle, dt, op, opname, kind, size, pool_t, pool_o)


@pytest.mark.parametrize('dtname,opname,kind,size',
                         [('MPI_INT8_T', 'MPI_SUM', 'int', 1), ('MPI_FLOAT', 'MPI_SUM', 'fp', 4),
                          ('MPI_INT64_T', 'MPI_MAX', 'int', 8)])
def test_looping_grid(R, H, oracle, dtname, opname, kind, size):
    """two one-wave blocks stride over the elements / the dwords"""
    dt, op = getattr(H, dtname), getattr(H, opname)
    pool_t, pool_o = c3_pools(kind, size, 0x5EED1720 + dt)
    before = R.get_launch()
    assert R.set_launch(64, 2) == 0
    try:
        run_parity(R, H, oracle, dt, op, opname, kind, size, pool_t, pool_o, counts=[257, 4099])
    finally:
        assert R.set_launch(before['block'], before['max_grid']) == 0
    assert R.get_launch() == before


# ------------------------------------------------------ concurrent callers
def run_threads(body, nthreads=NTHREADS):
    """body(t, stream) in host threads, each with a stream of its own, released
    together by a barrier; returns after every stream has drained"""
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(nthreads)]
    bar = threading.Barrier(nthreads)
    errs = []

    def work(t):
        try:
            torch.cuda.set_device(0)
            bar.wait(timeout=60)
            body(t, streams[t])
            streams[t].synchronize()
        except BaseException as e:      # noqa: BLE001  (reported by the caller)
            errs.append(repr(e))
            bar.abort()

    ths = [threading.Thread(target=work, args=(t,)) for t in range(nthreads)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=120)
    assert not errs, errs
    assert not any(th.is_alive() for th in ths)
    torch.cuda.synchronize()


def device_target(nbytes, phase, fill=0):
    """`nbytes` of device memory at byte `phase` past a 256-byte-aligned
    address, and the whole allocation around it"""
    raw = torch.full((nbytes + 512,), fill, dtype=torch.uint8, device='cuda')
    lo = (-raw.data_ptr()) % 256 + 64 + phase
    return raw[lo:lo + nbytes], raw, lo


TICKET_TYPES = [('MPI_INT8_T', torch.int8, 1), ('MPI_INT8_T', torch.int8, 3),
                ('MPI_INT16_T', torch.int16, 2), ('MPI_INT32_T', torch.int32, 0),
                ('MPI_INT64_T', torch.int64, 0), ('MPI_FLOAT', torch.float32, 4),
                ('MPI_DOUBLE', torch.float64, 8), ('MPIX_C_FLOAT16', torch.float16, 2)]


def check_tickets(results, target, tdt, calls):
    """per element: the fetched values, sorted, are 0 .. calls - 1, and the
    target holds their number (wrapped to the type in the target only)"""
    n = target.numel()
    got = results.reshape(calls, n).sort(0).values
    want = torch.arange(calls, device='cuda').to(tdt).reshape(calls, 1).expand(calls, n)
    assert torch.equal(got, want), 'the fetched values are not 0 .. %d' % (calls - 1)
    end = torch.tensor(calls, dtype=torch.int64).to(tdt).item()     # 128 wraps in int8
    assert bool((target == end).all()), 'the target is not %r everywhere' % end


@pytest.mark.parametrize('dtname,tdt,phase', TICKET_TYPES,
                         ids=['%s@%d' % (t[0], t[2]) for t in TICKET_TYPES])
def test_tickets(R, H, dtname, tdt, phase):
    dt, n = getattr(H, dtname), 16384
    ext = R.datatype_extent(dt)
    tb, raw, lo = device_target(n * ext, phase)
    target = tb.view(tdt)
    ones = torch.ones(n, dtype=tdt, device='cuda')
    results = torch.full((NTHREADS, CALLS, n), -1, dtype=tdt, device='cuda')

    def body(t, stream):
        for r in range(CALLS):
            assert R.get_accumulate_local_atomic(ones, results[t, r], target, n, dt, H.MPI_SUM,
                                                 stream=stream) == 0

    run_threads(body)
    check_tickets(results, target, tdt, NTHREADS * CALLS)
    assert bool((ones == 1).all())
    h = raw.cpu()
    assert bool((h[:lo] == 0).all() and (h[lo + n * ext:] == 0).all()), 'bytes around the target'


def test_adjacent_ranges_share_a_dword(R, H):
    """two callers on [0, 5) and [5, 10) of MPI_INT8_T: the dword [4, 8) belongs
    to both, neither loses the other's bytes"""
    tb, raw, lo = device_target(16, 0)
    target = tb.view(torch.int8)
    origins = [torch.full((5,), v, dtype=torch.int8, device='cuda') for v in (1, 2)]
    results = torch.full((2, CALLS, 5), -1, dtype=torch.int8, device='cuda')

    def body(t, stream):
        for r in range(CALLS):
            if r % 2:
                assert R.get_accumulate_local_atomic(origins[t], results[t, r],
                                                     target[5 * t:5 * t + 5], 5, H.MPI_INT8_T,
                                                     H.MPI_SUM, stream=stream) == 0
            else:
                assert R.accumulate_local_atomic(origins[t], target[5 * t:5 * t + 5], 5,
                                                 H.MPI_INT8_T, H.MPI_SUM, stream=stream) == 0

    run_threads(body, 2)
    want = [CALLS] * 5 + [2 * CALLS] * 5 + [0] * 6
    assert target.cpu().tolist() == want
    for t in range(2):      # one caller per range, stream-ordered: every second value
        got = results[t, 1::2].cpu()
        exp = torch.arange(1, CALLS, 2, dtype=torch.int8).reshape(-1, 1).expand(-1, 5) * (t + 1)
        assert torch.equal(got, exp)
    assert bool((raw.cpu() == 0).sum() == raw.numel() - 10)


# 3 ------------------------------------------------------------ swap chain
@pytest.mark.parametrize('dtname,tdt,phase', [('MPI_UINT8_T', torch.uint8, 1),
                                              ('MPI_INT16_T', torch.int16, 2),
                                              ('MPI_INT32_T', torch.int32, 4),
                                              ('MPI_INT64_T', torch.int64, 0)],
                         ids=['u8', 'i16', 'i32', 'i64'])
def test_swap_chain(R, H, dtname, tdt, phase):
    """MPI_REPLACE with a unique token per call: per element the fetched values
    and the final target are the tokens and the initial value, each once"""
    dt, n = getattr(H, dtname), 4096
    ext = R.datatype_extent(dt)
    tb, raw, lo = device_target(n * ext, phase)
    target = tb.view(tdt)
    tokens = (1 + torch.arange(NTHREADS * CALLS, device='cuda')).to(tdt)
    origins = tokens.reshape(NTHREADS, CALLS, 1).expand(NTHREADS, CALLS, n).contiguous()
    results = torch.zeros((NTHREADS, CALLS, n), dtype=tdt, device='cuda')

    def body(t, stream):
        for r in range(CALLS):
            assert R.get_accumulate_local_atomic(origins[t, r], results[t, r], target, n, dt,
                                                 H.MPI_REPLACE, stream=stream) == 0

    run_threads(body)
    total = NTHREADS * CALLS
    seen = torch.cat([results.reshape(total, n), target.reshape(1, n)]).sort(0).values
    want = torch.arange(total + 1, device='cuda').to(tdt).reshape(-1, 1).expand(total + 1, n)
    assert torch.equal(seen, want)


# 4 ------------------------------------------------------- order-free folds
FOLD_OPS = ['MPI_MAX', 'MPI_MIN', 'MPI_BOR', 'MPI_BXOR', 'MPI_BAND', 'MPI_LOR', 'MPI_PROD']
FOLD_TYPES = [('MPI_INT8_T', 1, 3), ('MPI_UINT16_T', 2, 2), ('MPI_INT32_T', 4, 0),
              ('MPI_UINT64_T', 8, 0)]


@pytest.mark.parametrize('opname', FOLD_OPS)
@pytest.mark.parametrize('dtname,size,phase', FOLD_TYPES, ids=[t[0] for t in FOLD_TYPES])
def test_order_free_folds(R, H, oracle, dtname, size, phase, opname):
    """commutative and associative in bits: whatever order the four streams'
    calls took, the target is the oracle's fold in one fixed order"""
    dt, op, n, per = getattr(H, dtname), getattr(H, opname), 4099, 4
    rng = np.random.default_rng(0x5EED1740 + 16 * size + FOLD_OPS.index(opname))
    init = rng.integers(0, 256, n * size, dtype=np.uint8)
    org = rng.integers(0, 256, (NTHREADS, per, n * size), dtype=np.uint8)
    # keep the result from saturating over the 16 folds: mostly-set bits for
    # BAND, sparse ones for BOR, odd factors for PROD (the low byte's bit 0)
    if opname == 'MPI_BAND':
        for _ in range(3):
            org |= rng.integers(0, 256, org.shape, dtype=np.uint8)
    if opname == 'MPI_BOR':
        for _ in range(4):
            org &= rng.integers(0, 256, org.shape, dtype=np.uint8)
    if opname == 'MPI_PROD':
        org[:, :, ::size] |= 1
    if opname == 'MPI_LOR':
        org[:, :, :(n // 2) * size] = 0
        init[:(n // 4) * size] = 0
    tb, raw, lo = device_target(n * size, phase, GUARD)
    tb.copy_(torch.from_numpy(init))
    dorg = torch.from_numpy(org).cuda()

    def body(t, stream):
        for r in range(per):
            assert R.accumulate_local_atomic(dorg[t, r], tb, n, dt, op, stream=stream) == 0

    run_threads(body)
    want = init.copy()
    for t in range(NTHREADS):
        for r in range(per):
            assert oracle.reduce_local(org[t, r].copy(), want, n, dt, op) == 0
    assert np.array_equal(tb.cpu().numpy(), want)
    h = raw.cpu().numpy()
    assert (h[:lo] == GUARD).all() and (h[lo + n * size:] == GUARD).all()
    assert np.array_equal(dorg.cpu().numpy(), org)


# 5 ------------------------------------------------------ compare-and-swap
CAS_TYPES = [('MPI_UINT8_T', torch.uint8, 1), ('MPI_INT16_T', torch.int16, 2),
             ('MPI_INT32_T', torch.int32, 4), ('MPI_INT64_T', torch.int64, 8)]


@pytest.mark.parametrize('dtname,tdt,size', CAS_TYPES, ids=[t[0] for t in CAS_TYPES])
def test_cas_increments(R, H, dtname, tdt, size):
    """the usual retry pattern from four threads: an atomic fetch, then the
    compare-and-swap to the fetched value + 1, retried until it took"""
    dt = getattr(H, dtname)
    phase = size if size < 4 else 0
    tb, raw, lo = device_target(size, phase, GUARD)
    tb.zero_()
    target = tb.view(tdt)
    per, limit = CALLS, 100000
    tries = [0] * NTHREADS

    def body(t, stream):
        # page-locked operands: the host writes and reads them without a stream
        o, c, z = (torch.zeros(1, dtype=tdt).pin_memory() for _ in range(3))
        done = 0
        while done < per:
            tries[t] += 1
            assert tries[t] < limit
            assert R.get_accumulate_local_atomic(None, z, target, 1, dt, H.MPI_NO_OP,
                                                 sync=True) == 0
            seen = int(z.item())
            c[0], o[0] = seen, seen + 1
            assert R.compare_and_swap_local_atomic(o, c, z, target, dt, sync=True) == 0
            done += int(z.item()) == seen

    run_threads(body)
    assert int(target.item()) == NTHREADS * per
    assert all(t >= per for t in tries)
    h = raw.cpu().numpy()       # the neighbours inside the dword included
    assert (h[:lo] == GUARD).all() and (h[lo + size:] == GUARD).all()


@pytest.mark.parametrize('dtname,tdt,size', CAS_TYPES, ids=[t[0] for t in CAS_TYPES])
def test_cas_parity_with_the_plain_entry(R, H, dtname, tdt, size):
    dt = getattr(H, dtname)
    rng = np.random.default_rng(0x5EED1750 + size)
    for rep in range(6):
        tgt = rng.integers(0, 256, size, dtype=np.uint8)
        org = rng.integers(0, 256, size, dtype=np.uint8)
        org[0] = tgt[0] ^ 0x3c
        cmp_ = tgt.copy() if rep % 2 == 0 else rng.integers(0, 256, size, dtype=np.uint8)
        if rep == 5:
            cmp_ = tgt.copy()
            cmp_[-1] ^= 0x80
        for tph in ([0, 1, 2, 3] if size == 1 else [0, 2] if size == 2 else [0, size]):
            for sync in (False, True):
                got = []
                for f in (R.compare_and_swap_local_atomic, R.compare_and_swap_local):
                    O, C = Placed(org, (tph + 1) % 4), Placed(cmp_, (tph + 3) % 4)
                    Z, T = Placed(np.full(size, CANARY, np.uint8), (tph + 2) % 4), Placed(tgt, tph)
                    torch.cuda.synchronize()
                    assert f(O.v, C.v, Z.v, T.v, dt, sync=sync) == 0
                    torch.cuda.synchronize()
                    assert np.array_equal(O.bytes(), org) and np.array_equal(C.bytes(), cmp_)
                    assert O.guards_intact() and C.guards_intact()
                    assert Z.guards_intact() and T.guards_intact()
                    got.append((Z.bytes(), T.bytes()))
                assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][0], tgt)
                assert np.array_equal(got[0][1], got[1][1])
                swapped = np.array_equal(cmp_, tgt)
                assert np.array_equal(got[0][1], org if swapped else tgt)


# 6 ----------------------------------------------------------- two processes
CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from mpich_amd import handles as H
from mpich_amd import redop as R
handle, off, n, calls, out = bytes.fromhex(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), \
    int(sys.argv[5]), sys.argv[6]
torch.cuda.set_device(0)
assert R.lib().MPIX_Redop_init() == 0
base = R.ipc_open(handle)
ones = torch.ones(n, dtype=torch.int32, device='cuda')
res = torch.full((calls, n), -1, dtype=torch.int32, device='cuda')
torch.cuda.synchronize()
print('ready', flush=True)
assert sys.stdin.readline().strip() == 'go'
for r in range(calls):
    rc = R.get_accumulate_local_atomic(ones, res[r], base + off, n, H.MPI_INT32_T, H.MPI_SUM)
    assert rc == 0, rc
torch.cuda.synchronize()
np.save(out, res.cpu().numpy())
assert R.ipc_close(base) == 0
print('done', flush=True)
'''


def test_two_processes_on_an_ipc_mapping(R, H, tmp_path):
    """the parent and two fresh child processes, which open the parent's target
    with MPIX_Ipc_open, draw tickets from one target"""
    n = 16384
    tb, raw, lo = device_target(n * 4, 0)
    target = tb.view(torch.int32)
    ones = torch.ones(n, dtype=torch.int32, device='cuda')
    results = torch.full((CALLS, n), -1, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    handle, off = R.ipc_export(target)
    outs = [str(tmp_path / ('child%d.npy' % k)) for k in range(2)]
    procs = [subprocess.Popen([sys.executable, '-c', CHILD, ROOT, handle.hex(), str(off), str(n),
                               str(CALLS), outs[k]], stdin=subprocess.PIPE,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k in range(2)]
    def stop(p, why):
        p.kill()
        pytest.fail('%s: %s' % (why, p.communicate()[1][-3000:]))

    try:
        for p in procs:         # each child has opened the mapping and made its buffers
            ready, _, _ = select.select([p.stdout], [], [], 120)
            if not ready or p.stdout.readline().strip() != 'ready':
                stop(p, 'a child did not get ready')
        for p in procs:
            p.stdin.write('go\n')
            p.stdin.flush()
        for r in range(CALLS):
            assert R.get_accumulate_local_atomic(ones, results[r], target, n, H.MPI_INT32_T,
                                                 H.MPI_SUM) == 0
        torch.cuda.synchronize()
        for p in procs:
            out, err = p.communicate(timeout=120)
            assert p.returncode == 0 and 'done' in out, err[-3000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    everyone = torch.cat([results] + [torch.from_numpy(np.load(o)).cuda() for o in outs])
    check_tickets(everyone, target, torch.int32, 3 * CALLS)


# 7 ---------------------------------------------------- refusals on the GPU
def test_refusals_leave_every_byte(R, H):
    n = 64
    org = torch.arange(n * 16, dtype=torch.uint8, device='cuda')
    res = torch.full((n * 16,), CANARY, dtype=torch.uint8, device='cuda')
    dev_t = torch.full((n * 16 + 16,), 7, dtype=torch.uint8, device='cuda')
    pinned = torch.full((n * 16,), 7, dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()

    def both(want, o, z, t, dt, op):
        for sync in (False, True):
            assert R.get_accumulate_local_atomic(o, z, t, n, dt, op, sync=sync) == want
            assert R.accumulate_local_atomic(o, t, n, dt, op, sync=sync) == want

    # a page-locked target: outside device scope
    both(H.MPI_ERR_BUFFER, org, res, pinned, H.MPI_INT, H.MPI_SUM)
    both(H.MPI_ERR_BUFFER, org, res, pinned, H.MPI_INT, H.MPI_REPLACE)
    # a declined 16-byte type on device memory
    both(H.MPI_ERR_TYPE, org, res, dev_t, H.MPI_DOUBLE_INT, H.MPI_MAXLOC)
    both(H.MPI_ERR_TYPE, org, res, dev_t, H.MPIR_INT128, H.MPI_SUM)
    both(H.MPI_ERR_TYPE, org, res, dev_t, H.MPI_C_DOUBLE_COMPLEX, H.MPI_REPLACE)
    # a device target off its extent's grid
    both(H.MPI_ERR_BUFFER, org, res, dev_t[4:], H.MPI_DOUBLE, H.MPI_SUM)
    both(H.MPI_ERR_BUFFER, org, res, dev_t[2:], H.MPI_FLOAT, H.MPI_MAX)
    both(H.MPI_ERR_BUFFER, org, res, dev_t[1:], H.MPI_INT16_T, H.MPI_SUM)
    # a pageable origin or result
    both(H.MPI_ERR_BUFFER, np.zeros(n * 16, np.uint8), res, dev_t, H.MPI_INT, H.MPI_SUM)
    assert R.get_accumulate_local_atomic(org, np.zeros(n * 16, np.uint8), dev_t, n, H.MPI_INT,
                                         H.MPI_SUM) == H.MPI_ERR_BUFFER
    # compare-and-swap: page-locked target, 16-byte type, misaligned target
    for sync in (False, True):
        assert R.compare_and_swap_local_atomic(org, org[16:], res, pinned, H.MPI_INT,
                                               sync=sync) == H.MPI_ERR_BUFFER
        assert R.compare_and_swap_local_atomic(org, org[16:], res, dev_t, H.MPIR_UINT128,
                                               sync=sync) == H.MPI_ERR_TYPE
        assert R.compare_and_swap_local_atomic(org, org[16:], res, dev_t[4:], H.MPI_INT64_T,
                                               sync=sync) == H.MPI_ERR_BUFFER
    torch.cuda.synchronize()
    assert bool((org.cpu() == torch.arange(n * 16, dtype=torch.uint8)).all())
    assert bool((res == CANARY).all()) and bool((dev_t == 7).all()) and bool((pinned == 7).all())
