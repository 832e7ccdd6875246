#!/usr/bin/env python3
"""Host wall time of MPIX_Iov_plan_create + MPIX_Iov_plan_free for ONE build of
libmpix_redop.so, no GPU needed (neither entry makes a HIP call): tables of
1 Ki, 64 Ki and 1 Mi runs of 3 double-complex elements in three residue groups
(offsets 0, 4 and 8 modulo 16 in turn, gaps between the runs so none merge).

usage: plan_host_cost.py LIBPATH LABEL
Per size the median [min, max] in ms over REPEATS create + free pairs after one
warm-up pair.  One JSON line.  To compare two builds, run this once per build in
alternating fresh processes and compare the medians of the processes' medians;
the spread of one build's own repeats is the allowance."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPEATS = 9
C_DOUBLE_COMPLEX = 0x4c001041
vp, aint, i32 = ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_int


def main():
    L = ctypes.CDLL(os.path.abspath(sys.argv[1]))
    L.MPIX_Iov_plan_create.argtypes = [aint, vp, vp, i32, ctypes.POINTER(vp)]
    L.MPIX_Iov_plan_free.argtypes = [ctypes.POINTER(vp)]
    L.MPIX_Iov_plan_info.argtypes = [vp] + [ctypes.POINTER(aint)] * 6
    rows = []
    for nrun in (1 << 10, 1 << 16, 1 << 20):
        k = np.arange(nrun, dtype=np.int64)
        offs = k * 128 + 4 * (k % 3)
        cnts = np.full(nrun, 3, np.int64)
        ms = []
        for rep in range(REPEATS + 1):
            plan = vp()
            t0 = time.perf_counter()
            rc = L.MPIX_Iov_plan_create(nrun, offs.ctypes.data, cnts.ctypes.data, C_DOUBLE_COMPLEX,
                                        ctypes.byref(plan))
            if rep == 0:
                v = [aint() for _ in range(6)]
                assert rc == 0 and L.MPIX_Iov_plan_info(plan, *[ctypes.byref(x) for x in v]) == 0
                assert (v[0].value, v[1].value) == (3 * nrun, nrun), [x.value for x in v]
                groups = v[2].value
                assert groups == 3
            rc2 = L.MPIX_Iov_plan_free(ctypes.byref(plan))
            t1 = time.perf_counter()
            assert rc == 0 and rc2 == 0
            if rep:
                ms.append(1e3 * (t1 - t0))
        rows.append(dict(runs=nrun, groups=groups, median_ms=round(statistics.median(ms), 4),
                         min_ms=round(min(ms), 4), max_ms=round(max(ms), 4)))
    print(json.dumps(dict(label=sys.argv[2], repeats=REPEATS, rows=rows)))


if __name__ == '__main__':
    main()
