#!/usr/bin/env python3
"""The element-atomic entries against the parent's way to the same guarantee,
in one process.  Every row is the median [min, max] over BATCHES batches.

  (a) one caller, fetch form, MPI_INT32_T SUM and MPI_FLOAT SUM at 1 element,
      64 KiB and 64 MiB: MPIX_Get_accumulate_local_atomic_async against
      MPIX_Get_accumulate_local_async -- the price of atomicity.  HIP events
      around a batch of back-to-back calls on one stream, per call; the
      bandwidth counts 4 N s bytes for both (origin and target read, target
      and result written).
  (b) four host threads on ONE target, the same pairs and sizes: each thread
      issues 64 atomic async fetch calls on a stream of its own and waits for
      it, against the four threads taking one host mutex around the
      synchronous MPIX_Get_accumulate_local (as posix_rma.h holds its mutex
      around the copy and the op).  Host wall time of the 4 x 64 calls from
      the release of the threads to the last join.
  (c) MPIX_Compare_and_swap_local_atomic against MPIX_Compare_and_swap_local,
      synchronous, one caller, MPI_INT64_T: host wall time per call.

usage: acc_atomic_rows.py [OUT.json]     (default profiles/acc_atomic_rows.json)"""
import json
import os
import statistics
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpich_amd import handles as H  # noqa: E402
from mpich_amd import redop as R  # noqa: E402

BATCHES = 5
NTHREADS, CALLS = 4, 64
SIZES = [('1 element', 1), ('64 KiB', (64 << 10) // 4), ('64 MiB', (64 << 20) // 4)]
PAIRS = [('MPI_INT32_T', torch.int32), ('MPI_FLOAT', torch.float32)]


def mmm(xs):
    return [statistics.median(xs), min(xs), max(xs)]


def ok(rc):
    if rc:
        raise RuntimeError('MPI error class %d' % rc)


def one_caller(L, dtname, tdt, n):
    dt, op = H.as_c_int(getattr(H, dtname)), H.as_c_int(H.MPI_SUM)
    org = torch.ones(n, dtype=tdt, device='cuda')
    tgt = torch.zeros(n, dtype=tdt, device='cuda')
    res = torch.empty(n, dtype=tdt, device='cuda')
    reps = 10 if n * 4 >= (1 << 20) else 200
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    args = (org.data_ptr(), res.data_ptr(), tgt.data_ptr(), n, dt, op, sp)
    out = {}
    forms = (('atomic', L.MPIX_Get_accumulate_local_atomic_async),
             ('plain', L.MPIX_Get_accumulate_local_async))
    per = {k: [] for k, _ in forms}
    with torch.cuda.stream(s):
        for _, f in forms:
            ok(f(*args))
        s.synchronize()
        for _ in range(BATCHES):
            for k, f in forms:          # alternately, batch by batch
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(reps):
                    ok(f(*args))
                e1.record(s)
                s.synchronize()
                per[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    for k, _ in forms:
        us = mmm(per[k])
        out[k] = dict(us_per_call=us, GBps=[4 * n * 4 / (u * 1e-6) / 1e9 for u in us])
    out['calls_per_batch'] = reps
    return out


def four_threads(L, dtname, tdt, n):
    dt, op = H.as_c_int(getattr(H, dtname)), H.as_c_int(H.MPI_SUM)
    org = torch.ones(n, dtype=tdt, device='cuda')
    tgt = torch.zeros(n, dtype=tdt, device='cuda')
    res = [torch.empty(n, dtype=tdt, device='cuda') for _ in range(NTHREADS)]
    streams = [torch.cuda.Stream() for _ in range(NTHREADS)]
    mutex = threading.Lock()
    torch.cuda.synchronize()

    def atomic(t):
        a = (org.data_ptr(), res[t].data_ptr(), tgt.data_ptr(), n, dt, op, streams[t].cuda_stream)
        for _ in range(CALLS):
            ok(L.MPIX_Get_accumulate_local_atomic_async(*a))
        streams[t].synchronize()

    def locked(t):
        a = (org.data_ptr(), res[t].data_ptr(), tgt.data_ptr(), n, dt, op)
        for _ in range(CALLS):
            with mutex:
                ok(L.MPIX_Get_accumulate_local(*a))

    def batch(body):
        bar = threading.Barrier(NTHREADS + 1)
        errs = []

        def work(t):
            torch.cuda.set_device(0)
            bar.wait()
            try:
                body(t)
            except Exception as e:      # noqa: BLE001
                errs.append(repr(e))

        ths = [threading.Thread(target=work, args=(t,)) for t in range(NTHREADS)]
        for th in ths:
            th.start()
        bar.wait()
        t0 = time.perf_counter()
        for th in ths:
            th.join()
        dt_ = time.perf_counter() - t0
        if errs:
            raise RuntimeError(errs[0])
        return dt_ * 1e3

    forms = (('atomic_async_4_streams', atomic), ('mutex_sync', locked))
    per = {k: [] for k, _ in forms}
    for _, body in forms:
        batch(body)                     # warm-up: streams, library state per thread
    for _ in range(BATCHES):
        for k, body in forms:
            per[k].append(batch(body))
    expect = NTHREADS * CALLS * 2 * (BATCHES + 1)
    assert float(tgt[0]) == expect and float(tgt[-1]) == expect, (float(tgt[0]), expect)
    return {k: dict(wall_ms_for_256_calls=mmm(per[k])) for k, _ in forms}


def cas(L):
    dt = H.as_c_int(H.MPI_INT64_T)
    o = torch.tensor([5], dtype=torch.int64, device='cuda')
    c = torch.tensor([0], dtype=torch.int64, device='cuda')
    z = torch.zeros(1, dtype=torch.int64, device='cuda')
    t = torch.zeros(1, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    args = (o.data_ptr(), c.data_ptr(), z.data_ptr(), t.data_ptr(), dt)
    reps = 200
    forms = (('atomic', L.MPIX_Compare_and_swap_local_atomic), ('plain', L.MPIX_Compare_and_swap_local))
    per = {k: [] for k, _ in forms}
    for _, f in forms:
        ok(f(*args))
    for _ in range(BATCHES):
        for k, f in forms:
            t0 = time.perf_counter()
            for _ in range(reps):
                ok(f(*args))
            per[k].append((time.perf_counter() - t0) * 1e6 / reps)
    return {k: dict(us_per_call=mmm(per[k])) for k, _ in forms}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles',
                                                                 'acc_atomic_rows.json')
    L = R.lib()
    ok(L.MPIX_Redop_init())
    rows = dict(method=__doc__.split('\n\n')[0], batches=BATCHES, build=R.build_info(),
                device=torch.cuda.get_device_name(0), one_caller={}, four_threads={})
    for dtname, tdt in PAIRS:
        for label, n in SIZES:
            key = '%s SUM, %s' % (dtname, label)
            rows['one_caller'][key] = one_caller(L, dtname, tdt, n)
            rows['four_threads'][key] = four_threads(L, dtname, tdt, n)
    rows['compare_and_swap_sync'] = cas(L)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(rows, f, indent=1)
        f.write('\n')
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
