#!/usr/bin/env python3
"""The fused get-accumulate against the reference's two passes, for ONE build
of libmpix_redop.so, in one process, 1 GiB per operand:

  (a) MPIX_Get_accumulate_local_async(origin, result, target)
  (b) hipMemcpyAsync(result <- target, device to device), then
      MPIX_Reduce_local_async(origin, target) -- what posix_rma.h:366-375 does
      (MPIR_Localcopy, then the op), through entries the fused form leaves alone

timed alternately, batch by batch, by HIP events on one stream after a warm-up
call of each: BATCHES batches of REPS back-to-back calls, the median batch and
the min-max spread of the batches per call.  (a) is rated on its 4 N s
algorithmic bytes, (b) on 5 N s.  The vector row: target (blocklen, stride) =
(1, 2) fp64 at 64 Mi elements against hipMemcpy2DAsync +
MPIX_Reduce_local_vector_async.  One JSON line.

usage: getacc_rows.py LIBPATH LABEL   (run once per build to compare builds,
e.g. the result-store policies: EXTRA_FLAGS=-DMPIX_GETACC_RESULT_STORE=n)

       getacc_rows.py LIBPATH LABEL iov [ROWS]
The iov-target rows (ROWS: letters of ABCD, default all), same method, the
forms timed in turn:
  A  fp64 SUM, 1,024 runs of 65,536 elements, gaps of a run's length (512 MiB
     packed)
  B  fp64 SUM, 131,072 runs of 512 elements (the same bytes, a 3 MiB table)
  C  fp64 SUM, runs of 8 elements, 8 Mi elements in all
  D  DOUBLE_INT MAXLOC, the raw iovec of a contiguous 32 Mi-element array
     ({value, int} segments, one run per element)
each as (fused) MPIX_Get_accumulate_local_iov[ec]_async, (two_launch) the
MPI_NO_OP gather of the same entry followed by MPIX_Reduce_local_iov[ec]_async,
(reduce) that reduce call alone, the kernel's floor at 3 of the fused form's 4
N s bytes, and, row A only, (memcpy_per_run) one hipMemcpyAsync per run
followed by the reduce call: what a caller had before these entries.  The
events bracket whole calls, so the host's table building shows wherever it
outlasts the kernels.  Compare builds by running once per build, e.g. the run
lookup: EXTRA_FLAGS=-DMPIX_GETACC_IOV_LOOKUP=n.

       getacc_rows.py LIBPATH LABEL plan [ROWS]
The same rows through a committed plan (MPIX_Iov_plan_*), same method: per row
(plan_fetch) MPIX_Get_accumulate_local_plan_async and (plan_reduce)
MPIX_Reduce_local_plan_async after MPIX_Iov_plan_prepare, each against its
yardstick on the same table, (iov_fetch) MPIX_Get_accumulate_local_iov[ec]_async
and (iov_reduce) MPIX_Reduce_local_iov[ec]_async; plus the host's wall time of
MPIX_Iov_plan_create[_iovec] and of MPIX_Iov_plan_prepare (median of 3), and
what MPIX_Iov_plan_info reports.  Compare the run lookups by running once per
build: EXTRA_FLAGS=-DMPIX_PLAN_LOOKUP=n.

       getacc_rows.py LIBPATH LABEL typed [ROWS]
Rows A and B with a derived datatype on all three sides
(MPIX_[Get_]accumulate_local_typed_async), same method.  The target and the
result have the row's runs; the origin holds the same element total in runs 3/2
as long (a shorter last one), so its cuts fall elsewhere.  Per row
(typed_fetch) and (typed_acc) after MPIX_Iov_plan_prepare[_packed], each
against the composition of the existing entries on the same buffers:
(comp_fetch) the MPI_NO_OP gather of the origin through its plan, the
packed-origin MPIX_Get_accumulate_local_plan_async, the MPI_REPLACE scatter of
the packed result through MPIX_Reduce_local_plan_async; (comp_acc) the gather,
then MPIX_Reduce_local_plan_async.  The typed forms are rated on 4 N s / 3 N s
algorithmic bytes, the compositions move 8 N s / 5 N s.  A form `holds` when it
is not slower than its composition by more than that composition's own batch
spread (max - min)."""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpich_amd import handles as H  # noqa: E402
import bench  # noqa: E402

BATCHES, REPS = 5, 3
D2D = 3     # hipMemcpyDeviceToDevice

vp, aint, i32 = ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_int
L = ctypes.CDLL(os.path.abspath(sys.argv[1]))
L.MPIX_Reduce_local_async.argtypes = [vp, vp, aint, i32, i32, vp]
L.MPIX_Reduce_local_vector_async.argtypes = [vp, vp, aint, aint, aint, i32, i32, vp]
L.MPIX_Get_accumulate_local_async.argtypes = [vp, vp, vp, aint, i32, i32, vp]
L.MPIX_Get_accumulate_local_vector_async.argtypes = [vp, vp, vp, aint, aint, aint, i32, i32, vp]
L.MPIX_Datatype_extent.argtypes = [i32]
L.MPIX_Datatype_extent.restype = aint
# the HIP runtime the library itself is linked to (a lookup through its handle)
L.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, i32, vp]
L.hipMemcpy2DAsync.argtypes = [vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.c_size_t,
                               ctypes.c_size_t, i32, vp]


def ok(rc, what):
    if rc:
        raise RuntimeError('%s: %d' % (what, rc))


def timed(fused, two_pass, stream):
    """per-call ms of both forms, batch by batch in turn"""
    fused()
    two_pass()
    stream.synchronize()
    ta, tb = [], []
    for _ in range(BATCHES):
        for f, out in ((fused, ta), (two_pass, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(REPS):
                f()
            e1.record(stream)
            stream.synchronize()
            out.append(e0.elapsed_time(e1) / REPS)
    return sorted(ta), sorted(tb)


def row(name, opname, nbytes_packed, ta, tb, **extra):
    ma, mb = ta[len(ta) // 2], tb[len(tb) // 2]
    return dict(type=name, op=opname,
                fused_ms=round(ma, 4), fused_spread_ms=[round(ta[0], 4), round(ta[-1], 4)],
                two_pass_ms=round(mb, 4), two_pass_spread_ms=[round(tb[0], 4), round(tb[-1], 4)],
                fused_TBs=round(4 * nbytes_packed / (ma * 1e-3) / 1e12, 3),
                two_pass_TBs=round(5 * nbytes_packed / (mb * 1e-3) / 1e12, 3),
                ratio=round(ma / mb, 4),
                wins=bool(ma < mb - (tb[-1] - tb[0])), **extra)


def fill(buf8, kind, seed):
    if kind == 'fp32':
        bench.fill_uniform(buf8.view(torch.float32), seed)
    elif kind == 'fp64':
        bench.fill_uniform(buf8.view(torch.float64), seed)
    elif kind == 'int8':
        g = torch.Generator(device=buf8.device)
        g.manual_seed(seed)
        buf8.view(torch.int8).random_(-128, 128, generator=g)
    elif kind == 'double_int':      # {double, int, 4 bytes padding}
        bench.fill_uniform(buf8.view(torch.float64), seed)
        g = torch.Generator(device=buf8.device)
        g.manual_seed(seed + 1)
        buf8.view(torch.int64).view(-1, 2)[:, 1].random_(0, 1 << 20, generator=g)
    else:                           # 'x87' / 'binary128' slots
        bench.fill_soft_slots(buf8, kind, seed)


ROWS = [('MPI_FLOAT', 'MPI_SUM', 'fp32'), ('MPI_DOUBLE', 'MPI_SUM', 'fp64'),
        ('MPI_INT8_T', 'MPI_MAX', 'int8'), ('MPI_C_DOUBLE_COMPLEX', 'MPI_PROD', 'fp64'),
        ('MPI_DOUBLE_INT', 'MPI_MAXLOC', 'double_int'), ('MPI_COMPLEX32', 'MPI_PROD', 'binary128')]


def timed_forms(forms, stream):
    """per-call ms of every form, batch by batch in turn: {name: sorted list}"""
    for f in forms.values():
        f()
    stream.synchronize()
    out = {k: [] for k in forms}
    for _ in range(BATCHES):
        for k, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(REPS):
                f()
            e1.record(stream)
            stream.synchronize()
            out[k].append(e0.elapsed_time(e1) / REPS)
    return {k: sorted(v) for k, v in out.items()}


def iov_row(name, tn, on, nruns, packed_bytes, t):
    med = {k: v[len(v) // 2] for k, v in t.items()}
    r = dict(row=name, type=tn, op=on, runs=nruns, packed_bytes=packed_bytes)
    for k, v in t.items():
        r[k + '_ms'] = round(med[k], 4)
        r[k + '_spread_ms'] = [round(v[0], 4), round(v[-1], 4)]
    r['fused_TBs'] = round(4 * packed_bytes / (med['fused'] * 1e-3) / 1e12, 3)
    r['ratio_to_two_launch'] = round(med['fused'] / med['two_launch'], 4)
    r['ratio_to_reduce'] = round(med['fused'] / med['reduce'], 4)
    spread = max(t['two_launch'][-1] - t['two_launch'][0], t['fused'][-1] - t['fused'][0])
    r['wins'] = bool(med['fused'] < med['two_launch'] - spread)
    return r


def iov_main():
    import numpy as np
    which = sys.argv[4] if len(sys.argv) > 4 else 'ABCD'
    iov_sig = [vp, vp, vp, aint, vp, vp, i32, i32, vp]
    L.MPIX_Get_accumulate_local_iov_async.argtypes = iov_sig
    L.MPIX_Get_accumulate_local_iovec_async.argtypes = iov_sig
    L.MPIX_Reduce_local_iov_async.argtypes = iov_sig[1:]
    L.MPIX_Reduce_local_iovec_async.argtypes = iov_sig[1:]
    dev = torch.device('cuda', 0)
    t8 = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    o8, r8 = (torch.empty(1 << 29, dtype=torch.uint8, device=dev) for _ in range(2))
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    tp, op_, rp = t8.data_ptr(), o8.data_ptr(), r8.data_ptr()
    no_op = H.as_c_int(H.MPI_NO_OP)
    rows = []
    shapes = dict(A=(1024, 65536), B=(131072, 512), C=(1 << 20, 8))
    for name in 'ABC':
        if name not in which:
            continue
        nruns, n = shapes[name]
        dt, op = H.as_c_int(H.MPI_DOUBLE), H.as_c_int(H.MPI_SUM)
        offs = (np.arange(nruns, dtype=np.int64) * (2 * n * 8))
        cnts = np.full(nruns, n, np.int64)
        po, pc = offs.ctypes.data, cnts.ctypes.data
        fill(t8, 'fp64', 0x5EED0B11)
        fill(o8, 'fp64', 0x5EED0B12)
        torch.cuda.synchronize()
        forms = {}

        def fused():
            ok(L.MPIX_Get_accumulate_local_iov_async(op_, rp, tp, nruns, po, pc, dt, op, sp),
               'MPIX_Get_accumulate_local_iov_async')

        def reduce():
            ok(L.MPIX_Reduce_local_iov_async(op_, tp, nruns, po, pc, dt, op, sp),
               'MPIX_Reduce_local_iov_async')

        def two_launch():
            ok(L.MPIX_Get_accumulate_local_iov_async(None, rp, tp, nruns, po, pc, dt, no_op, sp),
               'MPIX_Get_accumulate_local_iov_async NO_OP')
            reduce()
        forms.update(fused=fused, two_launch=two_launch, reduce=reduce)
        if name == 'A':
            def memcpy_per_run():
                for k in range(nruns):
                    ok(L.hipMemcpyAsync(rp + k * n * 8, tp + int(offs[k]), n * 8, D2D, sp),
                       'hipMemcpyAsync')
                reduce()
            forms['memcpy_per_run'] = memcpy_per_run
        rows.append(iov_row(name, 'MPI_DOUBLE', 'MPI_SUM', nruns, nruns * n * 8,
                            timed_forms(forms, s)))
    if 'D' in which:
        n = 32 << 20
        dt, op = H.as_c_int(H.MPI_DOUBLE_INT), H.as_c_int(H.MPI_MAXLOC)
        offs = np.empty(2 * n, np.int64)
        offs[0::2] = np.arange(n, dtype=np.int64) * 16
        offs[1::2] = offs[0::2] + 8
        lens = np.empty(2 * n, np.int64)
        lens[0::2], lens[1::2] = 8, 4
        po, pl = offs.ctypes.data, lens.ctypes.data
        fill(t8[:n * 16], 'double_int', 0x5EED0B13)
        fill(o8, 'double_int', 0x5EED0B14)
        torch.cuda.synchronize()

        def fused_d():
            ok(L.MPIX_Get_accumulate_local_iovec_async(op_, rp, tp, 2 * n, po, pl, dt, op, sp),
               'MPIX_Get_accumulate_local_iovec_async')

        def reduce_d():
            ok(L.MPIX_Reduce_local_iovec_async(op_, tp, 2 * n, po, pl, dt, op, sp),
               'MPIX_Reduce_local_iovec_async')

        def two_launch_d():
            ok(L.MPIX_Get_accumulate_local_iovec_async(None, rp, tp, 2 * n, po, pl, dt, no_op, sp),
               'MPIX_Get_accumulate_local_iovec_async NO_OP')
            reduce_d()
        rows.append(iov_row('D', 'MPI_DOUBLE_INT', 'MPI_MAXLOC', n, n * 16,
                            timed_forms(dict(fused=fused_d, two_launch=two_launch_d,
                                             reduce=reduce_d), s)))
    L.MPIX_Redop_build_info.restype = ctypes.c_char_p
    print(json.dumps(dict(label=sys.argv[2], lib=os.path.basename(sys.argv[1]),
                          build=L.MPIX_Redop_build_info().decode(), batches=BATCHES, reps=REPS,
                          rows=rows)))


def plan_row(name, tn, on, nseg, packed_bytes, t, info, create_ms, prepare_ms):
    med = {k: v[len(v) // 2] for k, v in t.items()}
    r = dict(row=name, type=tn, op=on, segments=nseg, packed_bytes=packed_bytes, **info,
             create_ms=round(create_ms, 3), prepare_ms=round(prepare_ms, 3))
    for k, v in t.items():
        r[k + '_ms'] = round(med[k], 4)
        r[k + '_spread_ms'] = [round(v[0], 4), round(v[-1], 4)]
    for form in ('fetch', 'reduce'):
        a, b = t['plan_' + form], t['iov_' + form]
        r[form + '_ratio_to_iov'] = round(med['plan_' + form] / med['iov_' + form], 4)
        spread = max(a[-1] - a[0], b[-1] - b[0])
        # not slower than its yardstick by more than the batches' spread
        r[form + '_holds'] = bool(med['plan_' + form] <= med['iov_' + form] + spread)
    r['plan_fetch_TBs'] = round(4 * packed_bytes / (med['plan_fetch'] * 1e-3) / 1e12, 3)
    r['plan_reduce_TBs'] = round(3 * packed_bytes / (med['plan_reduce'] * 1e-3) / 1e12, 3)
    return r


def plan_main():
    import time
    import numpy as np
    which = sys.argv[4] if len(sys.argv) > 4 else 'ABCD'
    iov_sig = [vp, vp, vp, aint, vp, vp, i32, i32, vp]
    L.MPIX_Get_accumulate_local_iov_async.argtypes = iov_sig
    L.MPIX_Get_accumulate_local_iovec_async.argtypes = iov_sig
    L.MPIX_Reduce_local_iov_async.argtypes = iov_sig[1:]
    L.MPIX_Reduce_local_iovec_async.argtypes = iov_sig[1:]
    L.MPIX_Iov_plan_create.argtypes = [aint, vp, vp, i32, ctypes.POINTER(vp)]
    L.MPIX_Iov_plan_create_iovec.argtypes = [aint, vp, vp, i32, ctypes.POINTER(vp)]
    L.MPIX_Iov_plan_prepare.argtypes = [vp, i32]
    L.MPIX_Iov_plan_info.argtypes = [vp] + [ctypes.POINTER(aint)] * 6
    L.MPIX_Iov_plan_free.argtypes = [ctypes.POINTER(vp)]
    L.MPIX_Reduce_local_plan_async.argtypes = [vp, vp, vp, i32, vp]
    L.MPIX_Get_accumulate_local_plan_async.argtypes = [vp, vp, vp, vp, i32, vp]
    dev = torch.device('cuda', 0)
    t8 = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    o8, r8 = (torch.empty(1 << 29, dtype=torch.uint8, device=dev) for _ in range(2))
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    tp, op_, rp = t8.data_ptr(), o8.data_ptr(), r8.data_ptr()
    shapes = dict(A=(1024, 65536), B=(131072, 512), C=(1 << 20, 8))
    rows = []
    for name in 'ABCD':
        if name not in which:
            continue
        if name == 'D':
            n = 32 << 20
            tn, on, kind, nseg, packed = 'MPI_DOUBLE_INT', 'MPI_MAXLOC', 'double_int', 2 * n, n * 16
            offs = np.empty(nseg, np.int64)
            offs[0::2] = np.arange(n, dtype=np.int64) * 16
            offs[1::2] = offs[0::2] + 8
            second = np.empty(nseg, np.int64)
            second[0::2], second[1::2] = 8, 4
            create, fetch, reduce = (L.MPIX_Iov_plan_create_iovec,
                                     L.MPIX_Get_accumulate_local_iovec_async,
                                     L.MPIX_Reduce_local_iovec_async)
            fill(t8[:packed], kind, 0x5EED0B13)
        else:
            nseg, n = shapes[name]
            tn, on, kind, packed = 'MPI_DOUBLE', 'MPI_SUM', 'fp64', nseg * n * 8
            offs = np.arange(nseg, dtype=np.int64) * (2 * n * 8)
            second = np.full(nseg, n, np.int64)
            create, fetch, reduce = (L.MPIX_Iov_plan_create, L.MPIX_Get_accumulate_local_iov_async,
                                     L.MPIX_Reduce_local_iov_async)
            fill(t8, kind, 0x5EED0B11)
        fill(o8, kind, 0x5EED0B12)
        dt, op = H.as_c_int(getattr(H, tn)), H.as_c_int(getattr(H, on))
        po, ps = offs.ctypes.data, second.ctypes.data
        torch.cuda.synchronize()
        plan, tc, tprep = vp(), [], []
        for _ in range(3):      # a fresh plan each time: prepare is idempotent on one
            if plan:
                ok(L.MPIX_Iov_plan_free(ctypes.byref(plan)), 'MPIX_Iov_plan_free')
            t0 = time.perf_counter()
            ok(create(nseg, po, ps, dt, ctypes.byref(plan)), 'MPIX_Iov_plan_create')
            t1 = time.perf_counter()
            ok(L.MPIX_Iov_plan_prepare(plan, 0), 'MPIX_Iov_plan_prepare')
            t2 = time.perf_counter()
            tc.append((t1 - t0) * 1e3)
            tprep.append((t2 - t1) * 1e3)
        v = [aint() for _ in range(6)]
        ok(L.MPIX_Iov_plan_info(plan, *[ctypes.byref(x) for x in v]), 'MPIX_Iov_plan_info')
        info = dict(elements=v[0].value, runs=v[1].value, groups=v[2].value,
                    table_bytes=v[5].value)

        def plan_fetch():
            ok(L.MPIX_Get_accumulate_local_plan_async(op_, rp, tp, plan, op, sp),
               'MPIX_Get_accumulate_local_plan_async')

        def iov_fetch():
            ok(fetch(op_, rp, tp, nseg, po, ps, dt, op, sp), 'the fetch entry')

        def plan_reduce():
            ok(L.MPIX_Reduce_local_plan_async(op_, tp, plan, op, sp), 'MPIX_Reduce_local_plan_async')

        def iov_reduce():
            ok(reduce(op_, tp, nseg, po, ps, dt, op, sp), 'the reduce entry')
        t = timed_forms(dict(plan_fetch=plan_fetch, iov_fetch=iov_fetch, plan_reduce=plan_reduce,
                             iov_reduce=iov_reduce), s)
        rows.append(plan_row(name, tn, on, nseg, packed, t, info, sorted(tc)[1], sorted(tprep)[1]))
        torch.cuda.synchronize()
        ok(L.MPIX_Iov_plan_free(ctypes.byref(plan)), 'MPIX_Iov_plan_free')
    L.MPIX_Redop_build_info.restype = ctypes.c_char_p
    print(json.dumps(dict(label=sys.argv[2], lib=os.path.basename(sys.argv[1]),
                          build=L.MPIX_Redop_build_info().decode(), batches=BATCHES, reps=REPS,
                          rows=rows)))


def typed_main():
    import numpy as np
    which = sys.argv[4] if len(sys.argv) > 4 else 'AB'
    L.MPIX_Iov_plan_create.argtypes = [aint, vp, vp, i32, ctypes.POINTER(vp)]
    L.MPIX_Iov_plan_prepare.argtypes = [vp, i32]
    L.MPIX_Iov_plan_prepare_packed.argtypes = [vp, i32]
    L.MPIX_Iov_plan_info.argtypes = [vp] + [ctypes.POINTER(aint)] * 6
    L.MPIX_Iov_plan_info_packed.argtypes = [vp, ctypes.POINTER(aint)]
    L.MPIX_Iov_plan_free.argtypes = [ctypes.POINTER(vp)]
    L.MPIX_Reduce_local_plan_async.argtypes = [vp, vp, vp, i32, vp]
    L.MPIX_Get_accumulate_local_plan_async.argtypes = [vp, vp, vp, vp, i32, vp]
    L.MPIX_Accumulate_local_typed_async.argtypes = [vp, vp, vp, vp, i32, vp]
    L.MPIX_Get_accumulate_local_typed_async.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp]
    dev = torch.device('cuda', 0)
    t8, o8, r8 = (torch.empty(1 << 30, dtype=torch.uint8, device=dev) for _ in range(3))
    po8, pr8 = (torch.empty(1 << 29, dtype=torch.uint8, device=dev) for _ in range(2))
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    tp, op_, rp, pop, prp = (x.data_ptr() for x in (t8, o8, r8, po8, pr8))
    dt = H.as_c_int(H.MPI_DOUBLE)
    op, no_op, replace = (H.as_c_int(x) for x in (H.MPI_SUM, H.MPI_NO_OP, H.MPI_REPLACE))
    shapes = dict(A=(1024, 65536), B=(131072, 512))
    rows = []

    def plan_of(lens):
        """runs of `lens` elements, each followed by a gap of its own length"""
        lens = np.asarray(lens, np.int64)
        offs = np.concatenate([[0], np.cumsum(2 * lens * 8)[:-1]]).astype(np.int64)
        assert int(offs[-1] + lens[-1] * 8) <= 1 << 30
        h = vp()
        ok(L.MPIX_Iov_plan_create(len(lens), offs.ctypes.data, lens.ctypes.data, dt,
                                  ctypes.byref(h)), 'MPIX_Iov_plan_create')
        return h

    for name in 'AB':
        if name not in which:
            continue
        nruns, n = shapes[name]
        total = nruns * n
        on = n * 3 // 2
        olens = [on] * (total // on) + ([total % on] if total % on else [])
        tplan, rplan, oplan = plan_of([n] * nruns), plan_of([n] * nruns), plan_of(olens)
        ok(L.MPIX_Iov_plan_prepare(tplan, 0), 'MPIX_Iov_plan_prepare')
        for h in (oplan, rplan):
            ok(L.MPIX_Iov_plan_prepare(h, 0), 'MPIX_Iov_plan_prepare')     # the composition's
            ok(L.MPIX_Iov_plan_prepare_packed(h, 0), 'MPIX_Iov_plan_prepare_packed')
        pk = aint()
        ok(L.MPIX_Iov_plan_info_packed(oplan, ctypes.byref(pk)), 'MPIX_Iov_plan_info_packed')
        fill(t8, 'fp64', 0x5EED0B21)
        fill(o8, 'fp64', 0x5EED0B22)
        torch.cuda.synchronize()

        def typed_fetch():
            ok(L.MPIX_Get_accumulate_local_typed_async(op_, oplan, rp, rplan, tp, tplan, op, sp),
               'MPIX_Get_accumulate_local_typed_async')

        def typed_acc():
            ok(L.MPIX_Accumulate_local_typed_async(op_, oplan, tp, tplan, op, sp),
               'MPIX_Accumulate_local_typed_async')

        def gather_origin():
            ok(L.MPIX_Get_accumulate_local_plan_async(None, pop, op_, oplan, no_op, sp),
               'the origin gather')

        def comp_fetch():
            gather_origin()
            ok(L.MPIX_Get_accumulate_local_plan_async(pop, prp, tp, tplan, op, sp),
               'MPIX_Get_accumulate_local_plan_async')
            ok(L.MPIX_Reduce_local_plan_async(prp, rp, rplan, replace, sp), 'the result scatter')

        def comp_acc():
            gather_origin()
            ok(L.MPIX_Reduce_local_plan_async(pop, tp, tplan, op, sp),
               'MPIX_Reduce_local_plan_async')
        t = timed_forms(dict(typed_fetch=typed_fetch, comp_fetch=comp_fetch, typed_acc=typed_acc,
                             comp_acc=comp_acc), s)
        med = {k: v[len(v) // 2] for k, v in t.items()}
        packed = total * 8
        r = dict(row=name, type='MPI_DOUBLE', op='MPI_SUM', packed_bytes=packed, target_runs=nruns,
                 result_runs=nruns, origin_runs=len(olens), origin_packed_table_bytes=pk.value)
        for k, v in t.items():
            r[k + '_ms'] = round(med[k], 4)
            r[k + '_spread_ms'] = [round(v[0], 4), round(v[-1], 4)]
        for form, nbytes in (('fetch', 4), ('acc', 3)):
            c = t['comp_' + form]
            r[form + '_ratio_to_comp'] = round(med['typed_' + form] / med['comp_' + form], 4)
            r[form + '_holds'] = bool(med['typed_' + form] <= med['comp_' + form] + (c[-1] - c[0]))
            r['typed_%s_TBs' % form] = round(nbytes * packed / (med['typed_' + form] * 1e-3) / 1e12,
                                             3)
        rows.append(r)
        torch.cuda.synchronize()
        for h in (tplan, rplan, oplan):
            ok(L.MPIX_Iov_plan_free(ctypes.byref(h)), 'MPIX_Iov_plan_free')
    L.MPIX_Redop_build_info.restype = ctypes.c_char_p
    print(json.dumps(dict(label=sys.argv[2], lib=os.path.basename(sys.argv[1]),
                          build=L.MPIX_Redop_build_info().decode(), batches=BATCHES, reps=REPS,
                          rows=rows)))


def main():
    nbytes = 1 << 30
    dev = torch.device('cuda', 0)
    t8, o8, r8 = (torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(3))
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    rows = []
    for tn, on, kind in ROWS:
        dt, op = H.as_c_int(getattr(H, tn)), H.as_c_int(getattr(H, on))
        ext = L.MPIX_Datatype_extent(dt)
        n = nbytes // ext
        fill(t8, kind, 0x5EED0B01)
        fill(o8, kind, 0x5EED0B02)
        torch.cuda.synchronize()

        def fused():
            ok(L.MPIX_Get_accumulate_local_async(o8.data_ptr(), r8.data_ptr(), t8.data_ptr(), n, dt,
                                                 op, sp), 'MPIX_Get_accumulate_local_async')

        def two_pass():
            ok(L.hipMemcpyAsync(r8.data_ptr(), t8.data_ptr(), n * ext, D2D, sp), 'hipMemcpyAsync')
            ok(L.MPIX_Reduce_local_async(o8.data_ptr(), t8.data_ptr(), n, dt, op, sp),
               'MPIX_Reduce_local_async')
        ta, tb = timed(fused, two_pass, s)
        rows.append(row(tn, on, n * ext, ta, tb, unit_bytes=ext))
    # vector target (1, 2) fp64, 64 Mi elements: target span 1 GiB, packed 512 MiB
    count = 64 << 20
    dt, op = H.as_c_int(H.MPI_DOUBLE), H.as_c_int(H.MPI_SUM)
    fill(t8, 'fp64', 0x5EED0B03)
    fill(o8, 'fp64', 0x5EED0B04)
    torch.cuda.synchronize()

    def fused_v():
        ok(L.MPIX_Get_accumulate_local_vector_async(o8.data_ptr(), r8.data_ptr(), t8.data_ptr(),
                                                    count, 1, 2, dt, op, sp),
           'MPIX_Get_accumulate_local_vector_async')

    def two_pass_v():
        ok(L.hipMemcpy2DAsync(r8.data_ptr(), 8, t8.data_ptr(), 16, 8, count, D2D, sp),
           'hipMemcpy2DAsync')
        ok(L.MPIX_Reduce_local_vector_async(o8.data_ptr(), t8.data_ptr(), count, 1, 2, dt, op, sp),
           'MPIX_Reduce_local_vector_async')
    try:
        ta, tb = timed(fused_v, two_pass_v, s)
        rows.append(row('MPI_DOUBLE vector(1,2)', 'MPI_SUM', count * 8, ta, tb, unit_bytes=8))
    except RuntimeError as e:       # e.g. a runtime that refuses a 2-D copy this tall
        rows.append(dict(type='MPI_DOUBLE vector(1,2)', op='MPI_SUM', error=str(e)))
    L.MPIX_Redop_build_info.restype = ctypes.c_char_p
    print(json.dumps(dict(label=sys.argv[2], lib=os.path.basename(sys.argv[1]),
                          build=L.MPIX_Redop_build_info().decode(), bytes_per_operand=nbytes,
                          batches=BATCHES, reps=REPS, rows=rows)))


if __name__ == '__main__':
    if len(sys.argv) > 3 and sys.argv[3] == 'iov':
        iov_main()
    elif len(sys.argv) > 3 and sys.argv[3] == 'plan':
        plan_main()
    elif len(sys.argv) > 3 and sys.argv[3] == 'typed':
        typed_main()
    else:
        main()
