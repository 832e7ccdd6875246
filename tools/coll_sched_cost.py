#!/usr/bin/env python3
"""Host cost of libmpix_coll's schedules alone: microseconds per call of one
rank on a null transport (a custom MPIX_XPORT_HOST communicator whose exchange
and combine functions return 0 at once, as tests/golden/make_coll_traces.py
drives it), so what is timed is the schedule's own index arithmetic, message
lists and bookkeeping.  No GPU, no threads.

Rows: every transport schedule at P = 8 and 16, blocks of 1 and 1001 MPI_INT
(allreduce / reduce / scan count = P blocks), rank 0 and rank P - 1.  A row is
the median over REPS batches of CALLS calls.  JSON to stdout.

    python tools/coll_sched_cost.py [--tree DIR]     # DIR: the checkout whose build is timed

Compare two builds in alternating processes (tools/README.md)."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPI_INT, MPI_SUM = 0x4c000405, 0x58000003
CALLS, REPS = 1000, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    from mpich_amd import ccl
    L = ccl.lib()
    xfn = ccl.EXCHANGE_FN(lambda ctx, rank, ops, nops, stream: 0)
    cfn = ccl.COMBINE_FN(lambda i, io, n, dt, op, stream: 0)
    rows = {}
    for P in (8, 16):
        for blk in (1, 1001):
            n = blk * P
            s = (ctypes.c_int * n)()
            r = (ctypes.c_int * n)()
            w = (ctypes.c_char * (4 * n * 4 + (1 << 16)))()
            for rank in (0, P - 1):
                h = ctypes.c_void_p()
                assert L.MPIX_Comm_create_custom(rank, P, ctypes.cast(xfn, ctypes.c_void_p), None,
                                                 ccl.XPORT_HOST, ctypes.byref(h)) == 0
                assert L.MPIX_Comm_set_combine(h, ctypes.cast(cfn, ctypes.c_void_p)) == 0
                calls = {}
                for alg in ('recursive_halving', 'pairwise', 'pairwise_sequential',
                            'recursive_halving_multipath'):
                    calls['rsb/' + alg] = lambda k=ccl.RSB_ALGORITHMS[alg]: \
                        L.MPIX_Reduce_scatter_block(s, r, blk, MPI_INT, MPI_SUM, h, k, w, len(w))
                for alg in ('reduce_scatter_allgather', 'rsag_rd_allgather', 'recursive_doubling',
                            'ring', 'rsag_multipath'):
                    calls['allreduce/' + alg] = lambda k=ccl.AR_ALGORITHMS[alg]: \
                        L.MPIX_Allreduce(s, r, n, MPI_INT, MPI_SUM, h, k, w, len(w))
                for alg, k in (('binomial', 1), ('scatter_gather', 2)):
                    calls['reduce/' + alg] = lambda k=k: \
                        L.MPIX_Reduce(s, r, n, MPI_INT, MPI_SUM, 0, h, k, w, len(w))
                calls['scan'] = lambda: L.MPIX_Scan(s, r, n, MPI_INT, MPI_SUM, h, w, len(w))
                for name, call in calls.items():
                    assert call() == 0, name
                    batches = []
                    for _ in range(REPS):
                        t0 = time.perf_counter()
                        for _ in range(CALLS):
                            call()
                        batches.append((time.perf_counter() - t0) / CALLS * 1e6)
                    batches.sort()
                    rows['%s P=%d block=%d rank=%d' % (name, P, blk, rank)] = \
                        round(batches[REPS // 2], 3)
                L.MPIX_Comm_free(h)
    print(json.dumps(dict(unit='us per call', calls=CALLS, reps=REPS, rows=rows)))


if __name__ == '__main__':
    main()
