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
e.g. the result-store policies: EXTRA_FLAGS=-DMPIX_GETACC_RESULT_STORE=n)"""
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
    main()
