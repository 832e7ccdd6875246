#!/usr/bin/env python3
"""Host cost per call of the RMA-style entries at sizes where it dominates (one
element and 64 KiB), two builds of libmpix_redop.so against each other in ONE
process: the process-to-process swing of such figures (where the process runs,
what it shares the box with) is about 1 us, several times what a host-side
change is likely to cost, and both builds in one process see the same.

usage: rma_host_cost.py PARENT_LIB BRANCH_LIB   (the same path twice: an A/A run)
Every row: bursts of BURST back-to-back calls on one stream, the host's wall
time of issuing a burst, per call, the builds taking turns burst by burst;
median [min, max] in us over BATCHES bursts of each after a warm-up burst.
The synchronous rows: wall time per call.  One JSON line."""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

BURST, BATCHES = 64, 30
vp, aint, i32 = ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_int
LIBS = [ctypes.CDLL(os.path.abspath(p)) for p in sys.argv[1:3]]
SUM, NO_OP, REPLACE = (ctypes.c_int(v - (1 << 32) if v >= 1 << 31 else v).value
                       for v in (0x58000003, 0x5800000e, 0x5800000d))
FLOAT, INT32, INT64 = 0x4c00040a, 0x4c000439, 0x4c00083a

SIG = {
    'MPIX_Redop_init': [],
    'MPIX_Get_accumulate_local_async': [vp, vp, vp, aint, i32, i32, vp],
    'MPIX_Get_accumulate_local': [vp, vp, vp, aint, i32, i32],
    'MPIX_Get_accumulate_local_vector_async': [vp, vp, vp, aint, aint, aint, i32, i32, vp],
    'MPIX_Reduce_local_vector_async': [vp, vp, aint, aint, aint, i32, i32, vp],
    'MPIX_Reduce_local_vector': [vp, vp, aint, aint, aint, i32, i32],
    'MPIX_Get_accumulate_local_iov_async': [vp, vp, vp, aint, vp, vp, i32, i32, vp],
    'MPIX_Iov_plan_create': [aint, vp, vp, i32, ctypes.POINTER(vp)],
    'MPIX_Iov_plan_prepare': [vp, i32],
    'MPIX_Reduce_local_plan_async': [vp, vp, vp, i32, vp],
    'MPIX_Get_accumulate_local_plan_async': [vp, vp, vp, vp, i32, vp],
    'MPIX_Get_accumulate_local_plan': [vp, vp, vp, vp, i32],
    'MPIX_Compare_and_swap_local_async': [vp, vp, vp, vp, i32, vp],
    'MPIX_Compare_and_swap_local': [vp, vp, vp, vp, i32],
    'MPIX_Accumulate_local_atomic_async': [vp, vp, aint, i32, i32, vp],
    'MPIX_Get_accumulate_local_atomic_async': [vp, vp, vp, aint, i32, i32, vp],
    'MPIX_Get_accumulate_local_atomic': [vp, vp, vp, aint, i32, i32],
    'MPIX_Compare_and_swap_local_atomic_async': [vp, vp, vp, vp, i32, vp],
    'MPIX_Compare_and_swap_local_atomic': [vp, vp, vp, vp, i32],
}
for L in LIBS:
    for name, args in SIG.items():
        getattr(L, name).argtypes = args
        getattr(L, name).restype = i32


def mmm(xs):
    return [round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]


def burst_once(name, f, args, stream):
    t0 = time.perf_counter()
    for _ in range(BURST):
        rc = f(*args)
    t1 = time.perf_counter()
    if stream is not None:
        stream.synchronize()
    if rc:
        raise RuntimeError('%s: MPI error class %d' % (name, rc))
    return 1e6 * (t1 - t0) / BURST


def ab_row(name, fname, args_of, stream):
    """args_of(k): the arguments for library k (its own plan handle)"""
    fs = [getattr(L, fname) for L in LIBS]
    for k in (0, 1):
        burst_once(name, fs[k], args_of(k), stream)
    xs = ([], [])
    for b in range(BATCHES):
        for k in ((0, 1) if b % 2 == 0 else (1, 0)):
            xs[k].append(burst_once(name, fs[k], args_of(k), stream))
    return dict(row=name, parent_us=mmm(xs[0]), branch_us=mmm(xs[1]))


def main():
    for L in LIBS:
        assert L.MPIX_Redop_init() == 0
    dev = torch.device('cuda', 0)
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    n = (64 << 10) // 4
    org = torch.ones(2 * n, dtype=torch.float32, device=dev)
    res = torch.zeros(2 * n, dtype=torch.float32, device=dev)
    tgt = torch.zeros(4 * n, dtype=torch.float32, device=dev)
    i_org = torch.ones(n, dtype=torch.int32, device=dev)
    i_res = torch.zeros(n, dtype=torch.int32, device=dev)
    i_tgt = torch.zeros(n, dtype=torch.int32, device=dev)
    w = torch.zeros(8, dtype=torch.int64, device=dev)       # origin, compare, result, target words
    torch.cuda.synchronize()
    o, r, t = org.data_ptr(), res.data_ptr(), tgt.data_ptr()
    io, ir, it_ = i_org.data_ptr(), i_res.data_ptr(), i_tgt.data_ptr()
    wo, wc, wr, wt = (w.data_ptr() + 16 * k for k in range(4))
    # 16 runs of n / 16 elements, gaps of a run's length
    nrun, run = 16, n // 16
    offs = (aint * nrun)(*[2 * k * run * 4 for k in range(nrun)])
    cnts = (aint * nrun)(*[run] * nrun)
    plans = []
    for L in LIBS:
        plan = vp()
        assert L.MPIX_Iov_plan_create(nrun, offs, cnts, FLOAT, ctypes.byref(plan)) == 0
        assert L.MPIX_Iov_plan_prepare(plan, 0) == 0
        plans.append(plan)
    PLAN = object()     # stands for the library's own plan handle
    iov = (ctypes.addressof(offs), ctypes.addressof(cnts))
    table = []          # (row, entry, arguments without the stream)
    for label, cnt in (('1 element', 1), ('64 KiB', n)):
        for opn, op in (('SUM', SUM), ('NO_OP', NO_OP), ('REPLACE', REPLACE)):
            table.append(('getacc %s %s' % (opn, label), 'MPIX_Get_accumulate_local',
                          (o, r, t, cnt, FLOAT, op)))
        table.append(('getacc atomic SUM %s' % label, 'MPIX_Get_accumulate_local_atomic',
                      (io, ir, it_, cnt, INT32, SUM)))
        table.append(('acc atomic SUM %s' % label, 'MPIX_Accumulate_local_atomic',
                      (io, it_, cnt, INT32, SUM)))
    table += [
        ('getacc vector(1,2) SUM 64 KiB', 'MPIX_Get_accumulate_local_vector',
         (o, r, t, n, 1, 2, FLOAT, SUM)),
        ('reduce vector(1,2) SUM 64 KiB', 'MPIX_Reduce_local_vector', (o, t, n, 1, 2, FLOAT, SUM)),
        ('reduce vector(1,2) REPLACE 64 KiB', 'MPIX_Reduce_local_vector',
         (o, t, n, 1, 2, FLOAT, REPLACE)),
        ('getacc iov 16 runs SUM 64 KiB', 'MPIX_Get_accumulate_local_iov',
         (o, r, t, nrun) + iov + (FLOAT, SUM)),
        ('getacc plan 16 runs SUM 64 KiB', 'MPIX_Get_accumulate_local_plan', (o, r, t, PLAN, SUM)),
        ('reduce plan 16 runs SUM 64 KiB', 'MPIX_Reduce_local_plan', (o, t, PLAN, SUM)),
        ('getacc plan 16 runs REPLACE 64 KiB', 'MPIX_Get_accumulate_local_plan',
         (o, r, t, PLAN, REPLACE)),
        ('reduce plan 16 runs REPLACE 64 KiB', 'MPIX_Reduce_local_plan', (o, t, PLAN, REPLACE)),
        ('compare-and-swap', 'MPIX_Compare_and_swap_local', (wo, wc, wr, wt, INT64)),
        ('compare-and-swap atomic', 'MPIX_Compare_and_swap_local_atomic', (wo, wc, wr, wt, INT64)),
    ]
    sync = [row for row in table
            if row[0] in ('getacc SUM 1 element', 'getacc atomic SUM 1 element',
                          'getacc plan 16 runs SUM 64 KiB', 'reduce vector(1,2) SUM 64 KiB',
                          'compare-and-swap', 'compare-and-swap atomic')]

    def args_of(args, tail):
        return lambda k: tuple(plans[k] if a is PLAN else a for a in args) + tail
    rows = []
    with torch.cuda.stream(s):
        for name, entry, args in table:
            rows.append(ab_row(name, entry + '_async', args_of(args, (sp,)), s))
    for name, entry, args in sync:
        rows.append(ab_row('sync ' + name, entry, args_of(args, ()), None))
    print(json.dumps(dict(burst=BURST, batches=BATCHES, rows=rows)), flush=True)


if __name__ == '__main__':
    main()
