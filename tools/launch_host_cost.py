#!/usr/bin/env python3
"""Host cost per call of the entries whose launchers plan through
redop_launch.h (contiguous, batch, multi-input, tree, get-accumulate, vector),
at sizes where the host part dominates (one element and 64 KiB), two builds of
libmpix_redop.so against each other in ONE process, as tools/rma_host_cost.py
does and for its reason: between processes the same call swings by about 1 us.

usage: launch_host_cost.py PARENT_LIB BRANCH_LIB   (the same build twice: an A/A run)
Every stream-ordered row: bursts of BURST back-to-back calls on one stream, the
host's wall time of issuing a burst, per call, the builds taking turns burst by
burst; median [min, max] in us over BATCHES bursts of each after WARM warm-up
bursts, and the branch / parent ratio of the medians.  The synchronous row: wall
time per call.  One JSON line."""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

BURST, BATCHES, WARM = 64, 60, 4
vp, aint, i32 = ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_int
LIBS = [ctypes.CDLL(os.path.abspath(p)) for p in sys.argv[1:3]]
SUM = ctypes.c_int(0x58000003).value
FLOAT = 0x4c00040a

SIG = {
    'MPIX_Redop_init': [],
    'MPIX_Reduce_local': [vp, vp, aint, i32, i32],
    'MPIX_Reduce_local_async': [vp, vp, aint, i32, i32, vp],
    'MPIX_Reduce_local_batch_async': [vp, vp, vp, i32, i32, i32, vp],
    'MPIX_Reduce_local_multi_async': [vp, i32, vp, aint, i32, i32, vp],
    'MPIX_Reduce_local_tree_async': [vp, i32, vp, aint, i32, i32, vp],
    'MPIX_Get_accumulate_local_async': [vp, vp, vp, aint, i32, i32, vp],
    'MPIX_Reduce_local_vector_async': [vp, vp, aint, aint, aint, i32, i32, vp],
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


def ab_row(name, fname, args, stream):
    fs = [getattr(L, fname) for L in LIBS]
    for k in (0, 1) * WARM:
        burst_once(name, fs[k], args, stream)
    xs = ([], [])
    for b in range(BATCHES):
        for k in ((0, 1) if b % 2 == 0 else (1, 0)):
            xs[k].append(burst_once(name, fs[k], args, stream))
    a, b = mmm(xs[0]), mmm(xs[1])
    return dict(row=name, parent_us=a, branch_us=b, ratio=round(b[0] / a[0], 4))


def main():
    for L in LIBS:
        assert L.MPIX_Redop_init() == 0
    dev = torch.device('cuda', 0)
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    n = (64 << 10) // 4
    bufs = [torch.ones(2 * n, dtype=torch.float32, device=dev) * 2.0 ** -20 for _ in range(18)]
    torch.cuda.synchronize()
    p = [b.data_ptr() for b in bufs]
    ptrs = lambda xs: (vp * len(xs))(*xs)
    in8, io8 = ptrs(p[0:8]), ptrs(p[8:16])
    in3 = ptrs(p[0:3])
    rows = []
    with torch.cuda.stream(s):
        for label, cnt in (('1 element', 1), ('64 KiB', n)):
            cnt8 = (aint * 8)(*[cnt] * 8)
            keep = (cnt8,)      # ctypes arrays stay alive over the bursts
            table = [
                ('reduce async', 'MPIX_Reduce_local_async', (p[0], p[8], cnt, FLOAT, SUM, sp)),
                ('batch k=8 async', 'MPIX_Reduce_local_batch_async',
                 (ctypes.addressof(in8), ctypes.addressof(io8), ctypes.addressof(cnt8), 8, FLOAT,
                  SUM, sp)),
                ('multi k=3 async', 'MPIX_Reduce_local_multi_async',
                 (ctypes.addressof(in3), 3, p[8], cnt, FLOAT, SUM, sp)),
                ('tree k=8 async', 'MPIX_Reduce_local_tree_async',
                 (ctypes.addressof(in8), 8, p[16], cnt, FLOAT, SUM, sp)),
                ('getacc async', 'MPIX_Get_accumulate_local_async',
                 (p[0], p[17], p[8], cnt, FLOAT, SUM, sp)),
                ('vector(1,2) async', 'MPIX_Reduce_local_vector_async',
                 (p[0], p[8], cnt, 1, 2, FLOAT, SUM, sp)),
            ]
            for name, entry, args in table:
                rows.append(ab_row('%s %s' % (name, label), entry, args, s))
            del keep
    for label, cnt in (('1 element', 1), ('64 KiB', n)):
        rows.append(ab_row('reduce sync %s' % label, 'MPIX_Reduce_local',
                           (p[0], p[8], cnt, FLOAT, SUM), None))
    print(json.dumps(dict(burst=BURST, batches=BATCHES, libs=sys.argv[1:3],
                          worst_ratio=max(r['ratio'] for r in rows), rows=rows)), flush=True)


if __name__ == '__main__':
    main()
