"""The split combiners (MPI_COMPLEX32 PROD, MPI_C_LONG_DOUBLE_COMPLEX PROD) under
concurrent callers.  They are the one place where two launches share host
state: k_contig32 records the units it declines in a word buffer and k_fixup32
recombines them from it (redop_kernels.h is_split), the buffer kept per device
and stream by the registry of redop_fixup.h.  A pair of another caller between
the two launches on the same stream, or on another stream over the same words,
leaves a unit uncombined (the tree form shows it: the output keeps slot 0's
value) or combines it twice (the in-place form).

Every thread has operands of its own whose declined sets differ -- thread 0
real values stored as complex (every unit declined), thread 1 no special value
at all, the others a few at the edges of the 64-unit words -- checks every
return code, and after the join every result and every operand that was only
read is compared with oracle.reduce_local, all 32 bytes of every unit.
tests/test_fixup_registry.py holds the registry's rules against a fake device;
these tests hold them on the real one."""
import threading

import numpy as np
import pytest
import torch

from tests import test_soft_fp as S
from tests.test_soft_fp_gpu import _oracle_prod, _same, _split_operands, dev

pytestmark = pytest.mark.gpu

TYPES = [S.COMPLEX32, S.C_LD_COMPLEX]
TYPE_IDS = ['complex32', 'c_long_double']


@pytest.fixture(scope='module')
def R():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from mpich_amd import redop
    assert redop.lib().MPIX_Redop_init() == 0
    return redop


def thread_operands(rng, dt, t, n, calls):
    """`calls` pairs of n units for thread t as one array each (the operation
    is element-wise: one oracle call covers them all)"""
    total = n * calls
    at = []
    if t >= 2:      # a few specials at word edges, other places for every thread
        for c in range(calls):
            at += [c * n + u for u in (0, 63 - (t & 1), 64, 127 + t, n - 1 - (t & 1))]
    a, b = _split_operands(rng, dt, total, sorted(set(at)))
    if t == 0:
        a[:, 16:] = 0
        b[:, 16:] = 0
    return a, b


_B1 = {}


def b1_jobs(oracle, dt):
    """4 threads x 64 pairs of 4,099 units and the oracle's products, made once per type"""
    if dt not in _B1:
        rng = np.random.default_rng(0x5EED0B10 + dt)
        _B1[dt] = []
        for t in range(4):
            a, b = thread_operands(rng, dt, t, 4099, 64)
            _B1[dt].append((a, b, _oracle_prod(oracle, dt, a, b)))
    return _B1[dt]


@pytest.mark.parametrize('stream', ['null', 'user'])
@pytest.mark.parametrize('dt', TYPES, ids=TYPE_IDS)
def test_one_stream_many_threads(R, oracle, dt, stream):
    """B1: 4 threads enqueue on one stream -- the null stream (handle 0) or
    one torch.cuda.Stream -- 64 in-place calls and 64 two-slot tree calls into
    separate outputs each, then one synchronise"""
    n, calls = 4099, 64
    jobs = b1_jobs(oracle, dt)
    user = torch.cuda.Stream() if stream == 'user' else None
    handle = user.cuda_stream if user else 0
    D = []
    for a, b, _ in jobs:
        D.append(dict(a=dev(a), b=dev(b), io=dev(a), out=torch.full((n * calls * 32,), 0x5A,
                                                                     dtype=torch.uint8, device='cuda')))
    torch.cuda.synchronize()
    errs = []
    start = threading.Barrier(len(jobs))

    def work(d):
        cut = lambda x, c: x[c * n * 32:(c + 1) * n * 32]
        start.wait()
        for c in range(calls):
            rc = R.reduce_local_async(cut(d['b'], c), cut(d['io'], c), n, dt, S.MPI_PROD, handle)
            rc2 = R.reduce_local_tree_async([cut(d['a'], c), cut(d['b'], c)], cut(d['out'], c), n,
                                            dt, S.MPI_PROD, handle)
            if rc or rc2:
                errs.append((c, rc, rc2))

    th = [threading.Thread(target=work, args=(d,)) for d in D]
    for t in th:
        t.start()
    for t in th:
        t.join()
    torch.cuda.synchronize()
    assert not errs, errs[:4]
    for t, (d, (a, b, want)) in enumerate(zip(D, jobs)):
        _same(d['io'].cpu().numpy(), want, n * calls, ('in place, combined twice?', t))
        _same(d['out'].cpu().numpy(), want, n * calls, ('tree, left uncombined?', t))
        assert np.array_equal(d['a'].cpu().numpy(), a.reshape(-1).view(np.uint8)), ('slot 0', t)
        assert np.array_equal(d['b'].cpu().numpy(), b.reshape(-1).view(np.uint8)), ('in', t)


@pytest.mark.parametrize('dt', TYPES, ids=TYPE_IDS)
def test_stream_per_thread(R, oracle, dt):
    """B2: hipStreamPerThread is one handle value (2) and another stream in
    every thread, so a buffer keyed on the handle alone would serve two
    streams at once.  The first thread enqueues 32 calls of 70,001 units and
    waits, without synchronising, while the second enqueues its 32; then one
    device synchronise, both threads still alive (their streams with them)."""
    n, calls, handle = 70001, 32, 2
    rng = np.random.default_rng(0x5EED0B20 + dt)
    jobs, D = [], []
    for t in range(2):
        a, b = thread_operands(rng, dt, 2 * t, n, calls)    # all declined / a few
        jobs.append((a, b, _oracle_prod(oracle, dt, a, b)))
        D.append(dict(io=dev(a), b=dev(b)))
    torch.cuda.synchronize()
    errs = []
    enqueued = [threading.Event(), threading.Event()]
    done = threading.Event()

    def work(t):
        d = D[t]
        if t:
            enqueued[0].wait()
        for c in range(calls):
            sl = slice(c * n * 32, (c + 1) * n * 32)
            rc = R.reduce_local_async(d['b'][sl], d['io'][sl], n, dt, S.MPI_PROD, handle)
            if rc:
                errs.append((t, c, rc))
        enqueued[t].set()
        done.wait()

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    enqueued[1].wait()
    torch.cuda.synchronize()
    done.set()
    for t in th:
        t.join()
    assert not errs, errs[:4]
    for t, (d, (a, b, want)) in enumerate(zip(D, jobs)):
        _same(d['io'].cpu().numpy(), want, n * calls, ('per-thread stream', t))
        assert np.array_equal(d['b'].cpu().numpy(), b.reshape(-1).view(np.uint8)), ('in', t)


def test_sync_entry_growth_and_finalize(R, oracle):
    """B3: tests/test_gpu_parity.py test_concurrent_callers for MPI_COMPLEX32
    PROD: 8 threads x 5 MPI_Reduce_local calls whose counts alternate between
    1,000 and 2^20 + 17 units (the larger needs more than the 64 KiB word
    buffer: every thread's buffer grows), each thread calling finalize at its
    end while others still run; then one call from this thread"""
    dt = S.COMPLEX32
    counts = [1000, (1 << 20) + 17, 1000, (1 << 20) + 17, 1000]
    rng = np.random.default_rng(0x5EED0B30)
    base = {}
    for n in sorted(set(counts)):
        a, b = _split_operands(rng, dt, n, [])
        base[n] = (a, b, _oracle_prod(oracle, dt, a, b))
    jobs = []
    for t in range(8):
        per = {}
        for n, (a0, b0, want0) in base.items():
            a, b, want = a0.copy(), b0.copy(), want0
            if t == 0:
                a[:, 16:] = 0
                b[:, 16:] = 0
                want = _oracle_prod(oracle, dt, a, b)
            elif t >= 2:    # specials at word edges, other places for every thread
                at = [0, 63, 64, 64 * t - 1, 64 * t, n - 1 - t]
                a[at], b[at] = _split_operands(rng, dt, len(at), range(len(at)))
                want = want0.reshape(n, 32).copy()      # element-wise: only those units change
                want[at] = _oracle_prod(oracle, dt, a[at], b[at]).reshape(-1, 32)
                want = want.reshape(-1)
            per[n] = (a, b, want)
        db = {n: dev(per[n][1]) for n in per}
        jobs.append([(n, dev(per[n][0]), db[n], per[n]) for n in counts])
    torch.cuda.synchronize()
    errs = []

    def work(calls):
        torch.cuda.set_device(0)
        for n, da, db, _ in calls:
            rc = R.MPI_Reduce_local(db, da, n, dt, S.MPI_PROD)
            if rc:
                errs.append((n, rc))
        R.finalize()

    th = [threading.Thread(target=work, args=(calls,)) for calls in jobs]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs[:4]
    for t, calls in enumerate(jobs):
        for i, (n, da, db, (a, b, want)) in enumerate(calls):
            _same(da.cpu().numpy(), want, n, ('thread', t, 'call', i))
            assert np.array_equal(db.cpu().numpy(), b.reshape(-1).view(np.uint8)), ('in', t, i)
    # the library is still usable from this thread after the others finalized
    n, _, db, (a, b, want) = jobs[3][1]
    da = dev(a)
    assert R.MPI_Reduce_local(db, da, n, dt, S.MPI_PROD) == 0
    _same(da.cpu().numpy(), want, n, 'after finalize')
