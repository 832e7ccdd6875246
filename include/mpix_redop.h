/*
 * mpix_redop.h -- C-ABI of the MI355X-native local reduction library
 * (libmpix_redop.so, built from mpich_amd/csrc/).
 *
 * This is the drop-in boundary for MPICH's local element-wise reduction:
 * every entry point below replaces one reference interface, cited as
 * reference-file:line (paths relative to the pmodels/mpich tree).
 *
 *   MPIX_Reduce_local        <- MPIR_Reduce_local
 *                               src/include/mpir_coll.h:62-63,
 *                               body src/mpi/coll/reduce_local/reduce_local.c:53-96
 *   MPIX_Reduce_local_async  <- same contract, enqueued on a caller HIP stream
 *                               (what the NBC engines need:
 *                               src/mpi/coll/transports/gentran/gentran_utils.c:157-167)
 *   MPIX_Redop_is_supported  <- MPIR_Typerep_reduce_is_supported
 *                               src/mpi/datatype/typerep/yaksa/typerep_yaksa_pack.c:218-271,
 *                               used by maint/gen_coll.py:546-547 for host staging
 *   MPIX_Op_table / MPIX_SUM.. <- MPIR_Op_table + MPIR_op_function
 *                               src/mpi/coll/op/oputil.c:10-27, src/include/mpir_op.h:206-209
 *   MPIX_Redop_op_dt_check   <- MPIR_op_dt_check  src/include/mpir_datatype.h:780-868
 *   MPIX_Redop_internal_op_dt_check <- MPIR_Internal_op_dt_check  mpir_datatype.h:870-933
 *   MPIX_Datatype_internal   <- MPIR_DATATYPE_REPLACE_BUILTIN  mpir_datatype.h:169-176
 *                               with the table of src/mpi/datatype/typeutil.c:29-109
 *   MPIX_Reduce_local_vector <- typerep_op_fallback on an MPI_Type_vector target
 *                               src/mpi/datatype/typerep/src/typerep_op.c:69-155
 *   MPIX_Get_accumulate_local <- the local step of MPI_Get_accumulate / MPI_Fetch_and_op:
 *                               MPIR_Localcopy + MPIDI_POSIX_compute_accumulate,
 *                               src/mpid/ch4/shm/posix/posix_rma.h:366-375, 756-767
 *   MPIX_Redop_set_fortran_booleans <- MPIR_Abi_set_fortran_booleans_impl
 *                               src/mpi/datatype/typeutil.c:502-515
 *
 * Handles use MPICH's own 32-bit encoding (src/include/mpi.h.in:166-311 and
 * src/include/mpir_datatype.h:22-125), so an MPICH build can pass its
 * MPI_Datatype / MPI_Op values straight through.  Both the external builtin
 * handles (MPI_FLOAT = 0x4c00040a) and the internal ones MPIR_Reduce_local
 * receives (MPIR_FLOAT32|0x0a = 0x4c83040a) are accepted, as are the struct
 * pair types MPI_{FLOAT,DOUBLE,LONG,SHORT}_INT (0x8c00000k).
 *
 * No C++ or torch types appear here: plain pointers, sizes and int codes.
 */
#ifndef MPIX_REDOP_H_INCLUDED
#define MPIX_REDOP_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int MPIX_Datatype;      /* same width/encoding as MPICH's MPI_Datatype */
typedef int MPIX_Op;            /* same width/encoding as MPICH's MPI_Op */
typedef intptr_t MPIX_Aint;     /* MPI_Aint on LP64 */

/* ---- return codes: MPI error classes (src/include/mpi.h.in:650-677) ---- */
#define MPIX_REDOP_SUCCESS     0
#define MPIX_REDOP_ERR_BUFFER  1        /* MPI_ERR_BUFFER: NULL / MPI_IN_PLACE / aliased */
#define MPIX_REDOP_ERR_COUNT   2        /* MPI_ERR_COUNT: negative count */
#define MPIX_REDOP_ERR_TYPE    3        /* MPI_ERR_TYPE: datatype unknown or not on GPU */
#define MPIX_REDOP_ERR_OP      9        /* MPI_ERR_OP: op undefined for this datatype */
#define MPIX_REDOP_ERR_ARG     12       /* MPI_ERR_ARG */
#define MPIX_REDOP_ERR_OTHER   15       /* MPI_ERR_OTHER: HIP runtime failure */
#define MPIX_REDOP_ERR_INTERN  16       /* MPI_ERR_INTERN */

/* ---- predefined ops (mpi.h.in:297-311); index = op & 0xf ---- */
#define MPIX_OP_NULL  ((MPIX_Op)0x18000000)
#define MPIX_MAX      ((MPIX_Op)0x58000001)
#define MPIX_MIN      ((MPIX_Op)0x58000002)
#define MPIX_SUM      ((MPIX_Op)0x58000003)
#define MPIX_PROD     ((MPIX_Op)0x58000004)
#define MPIX_LAND     ((MPIX_Op)0x58000005)
#define MPIX_BAND     ((MPIX_Op)0x58000006)
#define MPIX_LOR      ((MPIX_Op)0x58000007)
#define MPIX_BOR      ((MPIX_Op)0x58000008)
#define MPIX_LXOR     ((MPIX_Op)0x58000009)
#define MPIX_BXOR     ((MPIX_Op)0x5800000a)
#define MPIX_MINLOC   ((MPIX_Op)0x5800000b)
#define MPIX_MAXLOC   ((MPIX_Op)0x5800000c)
#define MPIX_REPLACE  ((MPIX_Op)0x5800000d)
#define MPIX_NO_OP    ((MPIX_Op)0x5800000e)
#define MPIX_EQUAL    ((MPIX_Op)0x5800000f)

/* ---- internal datatype encoding (mpir_datatype.h:22-125) ----
 * 0x4c | kind | size | builtin index.  Kinds: */
#define MPIX_TYPE_INTERNAL_MASK  0x800000
#define MPIX_TYPE_PAIR_MASK      0x400000
#define MPIX_TYPE_KIND_MASK      0x0f0000
#define MPIX_TYPE_FIXED          0x000000
#define MPIX_TYPE_SIGNED         0x010000
#define MPIX_TYPE_UNSIGNED       0x020000
#define MPIX_TYPE_FLOAT          0x030000
#define MPIX_TYPE_COMPLEX        0x040000
#define MPIX_TYPE_ALT_FLOAT      0x050000
#define MPIX_TYPE_ALT_COMPLEX    0x060000
#define MPIX_TYPE_FORTRAN_LOGICAL 0x070000

#define MPIX_INT8      ((MPIX_Datatype)0x4c810100)
#define MPIX_INT16     ((MPIX_Datatype)0x4c810200)
#define MPIX_INT32     ((MPIX_Datatype)0x4c810400)
#define MPIX_INT64     ((MPIX_Datatype)0x4c810800)
#define MPIX_INT128    ((MPIX_Datatype)0x4c811000)
#define MPIX_UINT8     ((MPIX_Datatype)0x4c820100)
#define MPIX_UINT16    ((MPIX_Datatype)0x4c820200)
#define MPIX_UINT32    ((MPIX_Datatype)0x4c820400)
#define MPIX_UINT64    ((MPIX_Datatype)0x4c820800)
#define MPIX_UINT128   ((MPIX_Datatype)0x4c821000)
#define MPIX_FLOAT16   ((MPIX_Datatype)0x4c830200)
#define MPIX_FLOAT32   ((MPIX_Datatype)0x4c830400)
#define MPIX_FLOAT64   ((MPIX_Datatype)0x4c830800)
#define MPIX_FLOAT128  ((MPIX_Datatype)0x4c831000)
#define MPIX_COMPLEX16 ((MPIX_Datatype)0x4c840400)  /* 2 x fp16 */
#define MPIX_COMPLEX32 ((MPIX_Datatype)0x4c840800)  /* float _Complex */
#define MPIX_COMPLEX64 ((MPIX_Datatype)0x4c841000)  /* double _Complex */
#define MPIX_COMPLEX128 ((MPIX_Datatype)0x4c842000) /* 2 x __float128 */
#define MPIX_BFLOAT16_INTERNAL ((MPIX_Datatype)0x4c850200)
#define MPIX_ALT_FLOAT128 ((MPIX_Datatype)0x4c851000)   /* x86-64 long double */
#define MPIX_ALT_COMPLEX128 ((MPIX_Datatype)0x4c862000) /* long double _Complex */
#define MPIX_FORTRAN_LOGICAL8   ((MPIX_Datatype)0x4c870100)
#define MPIX_FORTRAN_LOGICAL16  ((MPIX_Datatype)0x4c870200)
#define MPIX_FORTRAN_LOGICAL32  ((MPIX_Datatype)0x4c870400)
#define MPIX_FORTRAN_LOGICAL64  ((MPIX_Datatype)0x4c870800)
#define MPIX_FORTRAN_LOGICAL128 ((MPIX_Datatype)0x4c871000)
/* builtin pair types {T value; T loc} (mpir_datatype.h:111-125) */
#define MPIX_2INT8     ((MPIX_Datatype)0x4cc10200)
#define MPIX_2INT16    ((MPIX_Datatype)0x4cc10400)
#define MPIX_2INT32    ((MPIX_Datatype)0x4cc10800)
#define MPIX_2INT64    ((MPIX_Datatype)0x4cc11000)
#define MPIX_2UINT8    ((MPIX_Datatype)0x4cc20200)
#define MPIX_2UINT16   ((MPIX_Datatype)0x4cc20400)
#define MPIX_2UINT32   ((MPIX_Datatype)0x4cc20800)
#define MPIX_2UINT64   ((MPIX_Datatype)0x4cc21000)
#define MPIX_2FLOAT16  ((MPIX_Datatype)0x4cc30400)
#define MPIX_2FLOAT32  ((MPIX_Datatype)0x4cc30800)
#define MPIX_2FLOAT64  ((MPIX_Datatype)0x4cc31000)

/* ---- a few external builtin handles (mpi.h.in:166-264) ---- */
#define MPIX_MPI_CHAR          ((MPIX_Datatype)0x4c000101)
#define MPIX_MPI_INT           ((MPIX_Datatype)0x4c000405)
#define MPIX_MPI_LONG          ((MPIX_Datatype)0x4c000807)
#define MPIX_MPI_FLOAT         ((MPIX_Datatype)0x4c00040a)
#define MPIX_MPI_DOUBLE        ((MPIX_Datatype)0x4c00080b)
#define MPIX_MPI_BYTE          ((MPIX_Datatype)0x4c00010d)
#define MPIX_MPI_2INT          ((MPIX_Datatype)0x4c000816)
#define MPIX_MPI_C_FLOAT16     ((MPIX_Datatype)0x4c000246)
#define MPIX_MPI_BFLOAT16      ((MPIX_Datatype)0x4c00024c)
/* struct pair types, created by MPIR_Datatype_init_pairtypes (pairtypes.c:99-121) */
#define MPIX_MPI_FLOAT_INT       ((MPIX_Datatype)0x8c000000)
#define MPIX_MPI_DOUBLE_INT      ((MPIX_Datatype)0x8c000001)
#define MPIX_MPI_LONG_INT        ((MPIX_Datatype)0x8c000002)
#define MPIX_MPI_SHORT_INT       ((MPIX_Datatype)0x8c000003)
#define MPIX_MPI_LONG_DOUBLE_INT ((MPIX_Datatype)0x8c000004)

/* ---- library lifetime ----
 * init is optional (every entry point initialises lazily); finalize frees
 * the calling thread's streams and host-staging scratch, and those that
 * exited threads left in the reuse pool (a thread that exits without
 * finalizing hands its state to the next new thread). */
int MPIX_Redop_init(void);
int MPIX_Redop_finalize(void);

/* ---- the hot path ----
 * inoutbuf[i] = inoutbuf[i] OP inbuf[i] for i < count elements of
 * `datatype` (extent-strided, i.e. pair padding preserved).
 *
 * MPIX_Reduce_local: synchronous, like MPIR_Reduce_local.  Buffers may be
 * device memory (hipMalloc / managed) or host memory; host operands are
 * staged through device scratch with hipMemcpyAsync.  count == 0 is a
 * successful no-op (reduce_local.c:59-60).
 *
 * MPIX_Reduce_local_async: both buffers must be device-accessible; the
 * kernel is enqueued on `stream` (a hipStream_t, NULL = legacy default
 * stream) and the call returns without waiting.
 *
 * Threads: any number of threads may call any entry at once, and any number
 * may enqueue on one stream -- a user stream, the null stream, or
 * hipStreamPerThread (a stream of its own in every thread) -- with the same
 * results as the calls one after another in the stream's order.  The kernels
 * keep no state between launches, with one exception the library serialises
 * itself: MPI_PROD on MPI_COMPLEX32 and MPI_C_LONG_DOUBLE_COMPLEX runs as two
 * launches that share a per-stream device buffer (per stream and thread for
 * hipStreamPerThread); each such call holds that buffer's lock over both
 * enqueues, so no other thread's pair comes between them, and records an event
 * behind them, without which the buffer is never freed or replaced.
 * MPIX_Redop_finalize from one thread leaves other threads' calls alone, in
 * flight or enqueued: it frees buffers that are idle, waits for the events (not
 * the streams) behind buffers with work still queued, and leaves a buffer a caller holds
 * to that caller; the next such call on a stream makes a buffer again. */
int MPIX_Reduce_local(const void *inbuf, void *inoutbuf, MPIX_Aint count,
                      MPIX_Datatype datatype, MPIX_Op op);
int MPIX_Reduce_local_async(const void *inbuf, void *inoutbuf, MPIX_Aint count,
                            MPIX_Datatype datatype, MPIX_Op op, void *stream);

/* Derived (vector) target, packed source -- typerep_op.c:115-150 with the
 * target an MPI_Type_vector(count, blocklen, stride, basic_type):
 *   for b < count, j < blocklen:
 *     inout[b*stride + j] = inout[b*stride + j] OP in[b*blocklen + j]
 * (stride and blocklen in elements; gaps in the target are never written).
 * Device buffers only; the sync form waits on its stream. */
int MPIX_Reduce_local_vector_async(const void *inbuf, void *inoutbuf, MPIX_Aint count,
                                   MPIX_Aint blocklen, MPIX_Aint stride,
                                   MPIX_Datatype basic_type, MPIX_Op op, void *stream);
int MPIX_Reduce_local_vector(const void *inbuf, void *inoutbuf, MPIX_Aint count,
                             MPIX_Aint blocklen, MPIX_Aint stride,
                             MPIX_Datatype basic_type, MPIX_Op op);

/* ---- fused get-accumulate ----
 * The local step of MPI_Get_accumulate, MPI_Fetch_and_op (count 1), MPI_Get
 * with MPI_NO_OP and a swap with MPI_REPLACE: for i < count elements of
 * `datatype` at extent stride
 *     result[i] = target[i]                  (the value before the call)
 *     target[i] = target[i] OP origin[i]
 * as one stream-ordered step that reads the target once -- the reference
 * copies the target into the result and then applies the op under one lock
 * (posix_rma.h:366-375, 756-767; mpidig_rma_callbacks.c:806-820).  The target
 * is in the inout role and the origin in the in role: the target's bits are
 * those MPIX_Reduce_local_async(origin, target, ...) leaves.
 *
 * Padded pair types (DOUBLE_INT, LONG_INT, SHORT_INT, LONG_DOUBLE_INT): the
 * result receives the data fields only and keeps its own padding bytes, as
 * MPIR_Localcopy does; the target keeps its padding as in the reduction.
 * MPI_NO_OP: result = target, the target is neither combined nor written and
 * `origin` is not read (it may be NULL).  MPI_REPLACE: result = old target,
 * target = origin.  MPIX_EQUAL is refused (MPI_ERR_OP).
 *
 * Errors are those of the reduction's entries, all decided before any device
 * work: count < 0, a non-builtin op, an unknown type, an illegal (op, type),
 * NULL buffers, a span of 2^56 bytes or more; any overlap among the three byte
 * ranges is MPI_ERR_BUFFER; a legal pair without a kernel (bf16 other than
 * SUM) is MPI_ERR_TYPE and touches no buffer.  count == 0 succeeds without
 * looking at any pointer.
 *
 * The async forms take operands a kernel on `stream` can dereference (device
 * memory, page-locked host memory; pageable host memory is MPI_ERR_BUFFER)
 * and return without waiting.  The sync forms need a device-memory target, run
 * on the calling thread's library stream and return when the result and the
 * target are visible.
 *
 * Vector form: the target is MPI_Type_vector(count, blocklen, stride,
 * basic_type) as in MPIX_Reduce_local_vector_async, origin and result are
 * packed: for b < count, j < blocklen
 *     result[b*blocklen + j] = target[b*stride + j]
 *     target[b*stride + j]   = target[b*stride + j] OP origin[b*blocklen + j]
 * Gap elements of the target are neither loaded nor written; the target's
 * byte range for the overlap check is its span. */
int MPIX_Get_accumulate_local_async(const void *origin, void *result, void *target,
                                    MPIX_Aint count, MPIX_Datatype datatype, MPIX_Op op,
                                    void *stream);
int MPIX_Get_accumulate_local(const void *origin, void *result, void *target,
                              MPIX_Aint count, MPIX_Datatype datatype, MPIX_Op op);
int MPIX_Get_accumulate_local_vector_async(const void *origin, void *result, void *target,
                                           MPIX_Aint count, MPIX_Aint blocklen, MPIX_Aint stride,
                                           MPIX_Datatype basic_type, MPIX_Op op, void *stream);
int MPIX_Get_accumulate_local_vector(const void *origin, void *result, void *target,
                                     MPIX_Aint count, MPIX_Aint blocklen, MPIX_Aint stride,
                                     MPIX_Datatype basic_type, MPIX_Op op);

/* General derived target given as its flattened iov, packed source --
 * typerep_op_fallback (typerep_op.c:100-150) with the target's iov already
 * resolved to element runs: for s < nseg, in order, seg_counts[s] elements
 * (extent stride) at byte offset seg_offsets[s] of inoutbuf are combined
 * with the next seg_counts[s] elements of inbuf.  Offsets may be negative
 * (lb < 0) and need only the 4-byte alignment of the element loads (2 for
 * 2-byte types); runs must not overlap (MPI accumulate targets).  The
 * tables are host arrays, read before the call returns (the run table is
 * uploaded through pinned memory, asynchronously on `stream`; two table
 * slots are used in turn, so a call waits only for the kernels of the iov
 * call before the previous one, whose slot it takes over).
 * Device buffers. */
int MPIX_Reduce_local_iov_async(const void *inbuf, void *inoutbuf, MPIX_Aint nseg,
                                const MPIX_Aint *seg_offsets, const MPIX_Aint *seg_counts,
                                MPIX_Datatype basic_type, MPIX_Op op, void *stream);

/* The same fallback over the raw iov, as MPIR_Typerep_to_iov_offset gives
 * it (typerep_op.c:100-110): segment i is iov_lens[i] BYTES at byte offset
 * iov_offsets[i] of inoutbuf.  For a basic type each segment must hold
 * whole elements (the reference asserts, :147; here MPI_ERR_ARG).  For a
 * pair type whose size is below its extent (DOUBLE_INT, LONG_INT,
 * SHORT_INT: the padding splits each element into {value, int} segments)
 * segments are gathered until they hold curr_len >= size bytes, then
 * curr_len / size elements are combined at extent stride from the first
 * gathered segment, and a partial element left at a segment's end starts
 * the next run -- typerep_op.c:117-148 exactly. */
int MPIX_Reduce_local_iovec_async(const void *inbuf, void *inoutbuf, MPIX_Aint nseg,
                                  const MPIX_Aint *iov_offsets, const MPIX_Aint *iov_lens,
                                  MPIX_Datatype basic_type, MPIX_Op op, void *stream);

/* ---- fused get-accumulate on iov / iovec targets ----
 * MPI_Get_accumulate, MPI_Fetch_and_op, MPI_Get (MPI_NO_OP) and the swap
 * (MPI_REPLACE) on any derived target datatype: MPIR_Localcopy(target ->
 * result) followed by the iov walk of the accumulate (posix_rma.h:366-375,
 * typerep_op.c:100-150) as one stream-ordered step that reads each target
 * element once.  The target is described exactly as inoutbuf is for
 * MPIX_Reduce_local_iov_async / _iovec_async (byte offsets that may be
 * negative, the same 4-byte / 2-byte residue rule, the iovec form's gather of
 * typerep_op.c:117-148); origin and result are packed, in run order: for run s
 * and k < its count, with p = the elements of earlier runs + k
 *     result[p]                                  = target element at seg_offsets[s] + k*extent
 *     target element at seg_offsets[s] + k*extent = that element OP origin[p]
 * The target's bits are those MPIX_Reduce_local_iov[ec]_async(origin, target,
 * ...) leaves.  The result takes the type map only: padded pairs are stored
 * member by member, so the result keeps its own padding and the target its
 * padding and gap bytes.  MPI_NO_OP fetches only (origin not read, may be
 * NULL; the target is not written), MPI_REPLACE swaps, MPIX_EQUAL is
 * MPI_ERR_OP.  Either is one launch per residue class however many runs.
 *
 * Errors, all decided before any device work (the run-table upload included),
 * in this order: nseg < 0 (MPI_ERR_COUNT); NULL tables (MPI_ERR_BUFFER); a
 * negative count or length (MPI_ERR_COUNT; the iovec form looks up the type
 * first, MPI_ERR_TYPE); a basic type's segment holding a partial element
 * (iovec, MPI_ERR_ARG); an unknown type (MPI_ERR_TYPE); a non-builtin op, an
 * illegal (op, type) or MPIX_EQUAL (MPI_ERR_OP).  A total of zero elements
 * then succeeds without looking at any of the three pointers.  Otherwise: NULL
 * or MPI_IN_PLACE result / target, or origin unless the op is MPI_NO_OP
 * (MPI_ERR_BUFFER); a misaligned residue (MPI_ERR_ARG); a packed range or the
 * target's bounding range -- lowest run start to highest run end, zero-length
 * runs aside -- of 2^56 bytes or more (MPI_ERR_COUNT); any overlap among the
 * packed origin, the packed result and that bounding range (MPI_ERR_BUFFER); a
 * legal pair without a kernel (bf16 other than SUM: MPI_ERR_TYPE, no buffer
 * touched).  Last, an operand the stream's device cannot dereference is
 * MPI_ERR_BUFFER.  Runs overlapping one another remain the caller's contract.
 *
 * Async forms only; the table upload shares the reduce form's two slots and
 * synchronises on their events, so these calls cannot be captured in a graph. */
int MPIX_Get_accumulate_local_iov_async(const void *origin, void *result, void *target,
                                        MPIX_Aint nseg, const MPIX_Aint *seg_offsets,
                                        const MPIX_Aint *seg_counts, MPIX_Datatype basic_type,
                                        MPIX_Op op, void *stream);
int MPIX_Get_accumulate_local_iovec_async(const void *origin, void *result, void *target,
                                          MPIX_Aint nseg, const MPIX_Aint *iov_offsets,
                                          const MPIX_Aint *iov_lens, MPIX_Datatype basic_type,
                                          MPIX_Op op, void *stream);

/* ---- committed iov plans ----
 * What MPI_Type_commit is to a datatype: the run table of one (iov, basic type)
 * built once and kept, where the _iov_async / _iovec_async entries above rebuild
 * and upload it on every call.  A caller keeps one plan per (count, committed
 * datatype) beside the datatype's own iov cache.
 *
 * MPIX_Iov_plan_create takes the tables of MPIX_Reduce_local_iov_async,
 * MPIX_Iov_plan_create_iovec those of MPIX_Reduce_local_iovec_async (the
 * padded pairs' gather of typerep_op.c:117-148 included); both read them before
 * they return.  Host work only, no HIP call: a plan can be created, queried and
 * freed on a machine without a GPU.  Runs are produced as by those entries;
 * zero-length runs are dropped; consecutive runs in call order merge into one
 * when run k+1 starts at offset[k] + count[k] * extent (their packed elements
 * are consecutive by construction, so no result bit changes; runs adjacent in
 * memory but not consecutive in call order stay apart); the merged runs are
 * grouped by their offset modulo the extent, and each group gets one 32-bit
 * index per 256 packed elements for the kernels' run lookup.
 *
 * Everything that depends only on the table and the type is decided here, in
 * this order: nseg < 0, or above INT_MAX (the reference asserts,
 * typerep_op.c:111) (MPI_ERR_COUNT); NULL tables (MPI_ERR_BUFFER); a negative
 * count or length (MPI_ERR_COUNT; the iovec form looks up the type first,
 * MPI_ERR_TYPE); a basic type's segment holding a partial element (iovec,
 * MPI_ERR_ARG); an unknown type (MPI_ERR_TYPE); a residue off the 4-byte
 * (2-byte types: 2-byte) alignment (MPI_ERR_ARG); a packed range or bounding
 * range -- lowest run start to highest run end -- of 2^56 bytes or more
 * (MPI_ERR_COUNT); a NULL `plan` (MPI_ERR_ARG).  On any error *plan is NULL.
 * A table of zero elements is a valid plan.
 *
 * MPIX_Iov_plan_info reports (each pointer may be NULL) the packed elements,
 * the runs after merging, the residue groups, the target's bounding byte
 * range [lo_byte, hi_byte) relative to the target pointer (lo_byte may be
 * negative; both 0 for an empty plan) and the bytes of table one device holds
 * (0 for a plan of at most one run, which needs none).
 *
 * MPIX_Iov_plan_prepare copies the tables into the memory of `device` (-1: the
 * current one).  It blocks and may allocate; it is idempotent and thread-safe.
 * A launch on a device whose tables are missing prepares them itself first, so
 * ONLY CALLS MADE AFTER prepare FOR THEIR DEVICE are free of allocation, copies
 * and host synchronisation, and only those may be captured in a graph.  After
 * it a call makes no allocation, no copy, no event call and no wait, and any
 * number of threads and streams may use one plan at once: the plan is immutable
 * apart from its per-device table set, which sits behind a mutex.
 * One exception: a plan of exactly one run takes the contiguous entries' path
 * (below), and with it their one piece of shared state.  In the reduce form the
 * split combiners (the x87 and binary128 types' ops) use the per-(device,
 * stream) fixup buffer of MPIX_Reduce_local_async: every such call takes the
 * buffer's lock around its two launches and records an event after them, and
 * its first use on a stream, and a later call that needs a larger one,
 * allocate.  So for such a plan, type and op, run one
 * call of at least that size on the stream before capturing or relying on a
 * call not to block -- exactly what MPIX_Reduce_local_async itself asks for.
 * Every other single-run call, the fetch form included, holds to the rule.
 *
 * MPIX_Iov_plan_free releases the device tables (hipFree synchronises the
 * device) and the host tables and sets *plan = NULL; freeing a NULL plan is a
 * no-op.  Work still queued on the plan, and a captured graph that references
 * it, are the caller's to finish or drop first.  MPIX_Redop_finalize does not
 * free plans.
 *
 * MPIX_Reduce_local_plan* and MPIX_Get_accumulate_local_plan* do exactly what
 * MPIX_Reduce_local_iov[ec]_async and MPIX_Get_accumulate_local_iov[ec]_async do
 * given the table the plan was created from: the target, every gap and padding
 * byte included, is bit-identical; the result receives the type map only;
 * MPI_NO_OP fetches (origin may be NULL) and does nothing in the reduce form;
 * MPI_REPLACE swaps in the fetch form and scatters in the reduce form.  One
 * launch per residue group.  A plan of exactly one run takes the contiguous
 * entries' path (MPIX_Reduce_local_async, MPIX_Get_accumulate_local_async) with
 * the target at the run's offset.
 *
 * Checks, all before any device work, in this order: a NULL plan
 * (MPI_ERR_ARG); a non-builtin op, an illegal (op, plan type) or MPIX_EQUAL
 * (MPI_ERR_OP); a plan of zero elements then succeeds without looking at a
 * pointer; NULL or MPI_IN_PLACE operands, the origin exempt under MPI_NO_OP in
 * the fetch form (MPI_ERR_BUFFER); any overlap among the packed ranges and the
 * plan's bounding range, the reduce form checking source against target the
 * same way -- O(1) (MPI_ERR_BUFFER); a legal pair without a kernel (bf16 other
 * than SUM: MPI_ERR_TYPE); an operand the stream's device cannot dereference
 * (MPI_ERR_BUFFER).
 *
 * The async forms take what a kernel on `stream` can dereference.  The sync
 * forms need a device-memory target, run on the calling thread's library
 * stream and return when the results are visible, as
 * MPIX_Get_accumulate_local. */
typedef struct MPIX_Iov_plan_s *MPIX_Iov_plan;

int MPIX_Iov_plan_create(MPIX_Aint nseg, const MPIX_Aint *seg_offsets, const MPIX_Aint *seg_counts,
                         MPIX_Datatype basic_type, MPIX_Iov_plan *plan);
int MPIX_Iov_plan_create_iovec(MPIX_Aint nseg, const MPIX_Aint *iov_offsets,
                               const MPIX_Aint *iov_lens, MPIX_Datatype basic_type,
                               MPIX_Iov_plan *plan);
int MPIX_Iov_plan_prepare(MPIX_Iov_plan plan, int device);
int MPIX_Iov_plan_info(MPIX_Iov_plan plan, MPIX_Aint *elements, MPIX_Aint *runs, MPIX_Aint *groups,
                       MPIX_Aint *lo_byte, MPIX_Aint *hi_byte, MPIX_Aint *table_bytes);
int MPIX_Iov_plan_free(MPIX_Iov_plan *plan);

int MPIX_Reduce_local_plan_async(const void *inbuf, void *inoutbuf, MPIX_Iov_plan plan, MPIX_Op op,
                                 void *stream);
int MPIX_Reduce_local_plan(const void *inbuf, void *inoutbuf, MPIX_Iov_plan plan, MPIX_Op op);
int MPIX_Get_accumulate_local_plan_async(const void *origin, void *result, void *target,
                                         MPIX_Iov_plan plan, MPIX_Op op, void *stream);
int MPIX_Get_accumulate_local_plan(const void *origin, void *result, void *target,
                                   MPIX_Iov_plan plan, MPIX_Op op);

/* ---- a datatype on every side: typed accumulate and get-accumulate ----
 * MPI_Accumulate and MPI_Get_accumulate (MPI_Put and MPI_Get are their
 * MPI_REPLACE / MPI_NO_OP cases) carry a datatype for the origin, the result
 * and the target.  The reference packs a derived origin into a buffer of its
 * own before the op (posix_rma.h:39-74: MPL_malloc, MPIR_Typerep_pack,
 * MPIR_Typerep_op) and serves a derived result with MPIR_Localcopy (:366).
 * Here each side is a committed plan and the call is one pass: no scratch
 * buffer, every element read or written once.
 *
 * For every packed index p < elements, in each plan's own call order:
 *   result element p = target element p (its value before the call)
 *   target element p = target element p OP origin element p
 * with the target in the inout role and the origin in the in role of the
 * combiner, exactly as in every other entry.  MPIX_Accumulate_local_typed* has
 * no result.  The result receives the type map only (padded pairs member by
 * member); result, target and origin keep their own padding and gap bytes,
 * which are never loaded or stored.
 *
 * A NULL origin_plan or result_plan means that operand is packed; with both
 * NULL the call leaves exactly the bits of MPIX_Reduce_local_plan* /
 * MPIX_Get_accumulate_local_plan*.  One plan handle may serve several roles of
 * one call.  MPI_NO_OP: the accumulate form does nothing; the fetch form is
 * MPI_Get into a derived result, and neither origin nor origin_plan is looked
 * at.  MPI_REPLACE: the accumulate form is MPI_Put with derived origin and
 * target, the fetch form the swap.  MPIX_EQUAL is no accumulate op.
 *
 * The packed-order table.  A plan's device table is grouped by residue and
 * driven from the target side; finding packed element p of the origin or the
 * result needs one table over all merged runs in call order: the packed
 * elements before each run, each run's byte offset, and one 32-bit run index
 * per 256 packed elements.  It is built with the plan (host work only) and is a
 * per-device allocation of its own, beside the tables MPIX_Iov_plan_info
 * reports.  A plan of at most one run keeps none.
 *   MPIX_Iov_plan_locate        the byte offset, relative to the buffer
 *     pointer, of packed element packed_index, through the lookup function the
 *     kernels use.  Host only, no HIP call.  A NULL plan or byte_offset is
 *     MPI_ERR_ARG, an index outside [0, elements) MPI_ERR_COUNT.
 *   MPIX_Iov_plan_info_packed   the bytes of packed-order table one device
 *     holds: (2 runs + 1) * 8 + (ceil(elements / 256) + 1) * 4, or 0 for a plan
 *     of at most one run.
 *   MPIX_Iov_plan_prepare_packed copies that table to `device` (-1: the current
 *     one): blocking, idempotent and thread-safe like MPIX_Iov_plan_prepare.  A
 *     launch that finds the table of an origin or result plan missing uploads it
 *     itself first.  So ONLY CALLS MADE AFTER prepare_packed FOR THE ORIGIN AND
 *     RESULT PLANS AND AFTER MPIX_Iov_plan_prepare FOR THE TARGET PLAN are free
 *     of allocation, copies and waits, and only those may be captured in a
 *     graph.  MPIX_Iov_plan_free releases it.
 *
 * Checks, all before any device work, in this order:
 *   1. a NULL target_plan (MPI_ERR_ARG);
 *   2. a non-builtin op, an illegal (op, target plan type) or MPIX_EQUAL
 *      (MPI_ERR_OP);
 *   3. every examined non-NULL plan, the origin's and then the result's (the
 *      origin's is not examined under MPI_NO_OP): an internal type other than
 *      the target plan's (MPI_ERR_TYPE), then an element count other than its
 *      (MPI_ERR_COUNT) -- MPI requires matching type signatures;
 *   4. zero elements then succeeds without looking at a pointer;
 *   5. NULL or MPI_IN_PLACE operands, the origin exempt under MPI_NO_OP
 *      (MPI_ERR_BUFFER);
 *   6. any pairwise overlap among the three BOUNDING byte ranges -- each plan's
 *      [lo_byte, hi_byte), or the packed range where the plan is NULL
 *      (MPI_ERR_BUFFER).  O(1); it refuses interleaved layouts whose bytes do not
 *      actually overlap, which is the rule the target already follows in the
 *      plan entries.  Runs overlapping one another inside the result or the
 *      target layout remain the caller's contract;
 *   7. a legal pair without a kernel (bf16 other than SUM: MPI_ERR_TYPE);
 *   8. an operand the stream's device cannot dereference (MPI_ERR_BUFFER).
 *
 * One launch per residue group of the TARGET plan.  When every side is packed
 * or one run, the call goes down the contiguous entries' path
 * (MPIX_Reduce_local_async, MPIX_Get_accumulate_local_async) with each buffer
 * at its run's offset, and the note above about the split combiners' per-stream
 * fixup buffer applies to the accumulate form again.
 *
 * The async forms take what a kernel on `stream` can dereference.  The sync
 * forms need a device-memory target, run on the calling thread's library
 * stream and return when target and result are visible, as
 * MPIX_Get_accumulate_local_plan. */
int MPIX_Iov_plan_locate(MPIX_Iov_plan plan, MPIX_Aint packed_index, MPIX_Aint *byte_offset);
int MPIX_Iov_plan_prepare_packed(MPIX_Iov_plan plan, int device);
int MPIX_Iov_plan_info_packed(MPIX_Iov_plan plan, MPIX_Aint *table_bytes);

int MPIX_Accumulate_local_typed_async(const void *origin, MPIX_Iov_plan origin_plan,
                                      void *target, MPIX_Iov_plan target_plan,
                                      MPIX_Op op, void *stream);
int MPIX_Accumulate_local_typed(const void *origin, MPIX_Iov_plan origin_plan,
                                void *target, MPIX_Iov_plan target_plan, MPIX_Op op);
int MPIX_Get_accumulate_local_typed_async(const void *origin, MPIX_Iov_plan origin_plan,
                                          void *result, MPIX_Iov_plan result_plan,
                                          void *target, MPIX_Iov_plan target_plan,
                                          MPIX_Op op, void *stream);
int MPIX_Get_accumulate_local_typed(const void *origin, MPIX_Iov_plan origin_plan,
                                    void *result, MPIX_Iov_plan result_plan,
                                    void *target, MPIX_Iov_plan target_plan, MPIX_Op op);

/* ---- compare-and-swap ----
 * The local step of MPI_Compare_and_swap on one element (posix_rma.h:605-608,
 * mpidig_rma_callbacks.c:1059-1068):
 *     *result = *target;  if (*compare == *target) *target = *origin;
 * compared as integers of the element's size.  Legal types are those of
 * MPIR_Type_is_rma_atomic (rmatypeutil.c:18-30): MPIX_Datatype_internal(
 * datatype) is one of MPIX_INT8..INT128, MPIX_UINT8..UINT128; anything else
 * (floating types, pairs, Fortran logicals) is MPI_ERR_TYPE and touches no
 * buffer.  NULL or MPI_IN_PLACE in any of the four pointers, result
 * overlapping any of the other three, or target overlapping origin or compare
 * is MPI_ERR_BUFFER; origin and compare may be the same address.  No operand
 * needs any alignment.
 *
 * Stream-ordered like every other entry, by plain loads and stores: atomicity
 * against other streams or processes is the window lock's business, as in the
 * reference, which holds a mutex around these lines.  The async form takes
 * operands a kernel on `stream` can dereference (pageable host memory is
 * MPI_ERR_BUFFER); the sync form needs a device-memory target, runs on the
 * calling thread's library stream and returns when result and target are
 * visible. */
int MPIX_Compare_and_swap_local_async(const void *origin, const void *compare, void *result,
                                      void *target, MPIX_Datatype datatype, void *stream);
int MPIX_Compare_and_swap_local(const void *origin, const void *compare, void *result,
                                void *target, MPIX_Datatype datatype);

/* ---- element-atomic accumulate, fetch-and-op and compare-and-swap ----
 * MPI's guarantee for concurrent accumulates to one target element with the
 * same predefined type, without a lock around the call: for every i < count
 *     target[i] = target[i] OP origin[i]
 * is ONE atomic read-modify-write at device scope on the 32- or 64-bit word
 * that holds the element, and in the fetch form result[i] is the value the
 * element had before that step.  The reference gets this from one mutex on its
 * shared-memory path (posix_rma.h:361-378) and from hardware atomics on its
 * network path where the (type, op) table allows (ofi_rma.h:67-132, 777-790);
 * this is the second way.
 *
 * The step is atomic with respect to every other call of these entries (any
 * op, on a type of the same extent), from any stream or thread, and from any
 * process that has the target mapped on the same device (MPIX_Ipc_open).
 * It is NOT atomic against the other, non-atomic entries of this header
 * (plain loads and stores: keep the window's lock between the two kinds), and
 * NOT across devices: a peer GPU's or the host's accesses to the target are
 * outside device scope.  The calls stay stream-ordered: the async forms
 * allocate nothing, record no event and wait for nothing.
 *
 * The combine is that of MPIX_Get_accumulate_local_async (target in the inout
 * role, origin in the in role): a caller that runs alone gets the same target
 * and result bits, NaNs, signed zeros, denormals, the bf16 store rule, Annex G
 * and pair padding included.  MPI_NO_OP is an atomic fetch (origin not read,
 * may be NULL; in the non-fetch form it does nothing); MPI_REPLACE an atomic
 * exchange, in the non-fetch form an atomic store per element; MPIX_EQUAL is
 * MPI_ERR_OP.
 *
 * Checks, all before any device work and in this order: those of
 * MPIX_Get_accumulate_local_async (count < 0, MPIX_EQUAL, a non-builtin op, an
 * unknown type, an illegal pair, count == 0 succeeds without looking at a
 * pointer, the 2^56-byte cap, NULL / MPI_IN_PLACE buffers, any overlap among
 * the byte ranges), then MPI_ERR_TYPE for a pair MPIX_Accumulate_atomic_is_
 * supported declines -- no kernel (bf16 other than SUM) or an extent of 16 or
 * 32 bytes (__int128, DOUBLE_INT, LONG_INT, the 2 x 64-bit pairs, double
 * complex, every long double / binary128 type): keep the lock and the
 * non-atomic entry for those -- then MPI_ERR_BUFFER for a target that is not
 * aligned to its extent.  Then, MPI_ERR_BUFFER as well: a target that is not
 * device memory of the stream's device (page-locked host memory, managed
 * memory, a peer device).  Origin and result are operands a kernel on `stream`
 * can dereference, element-aligned.  The sync forms run on the calling
 * thread's library stream and return when target and result are visible. */
int MPIX_Accumulate_local_atomic_async(const void *origin, void *target, MPIX_Aint count,
                                       MPIX_Datatype datatype, MPIX_Op op, void *stream);
int MPIX_Accumulate_local_atomic(const void *origin, void *target, MPIX_Aint count,
                                 MPIX_Datatype datatype, MPIX_Op op);
int MPIX_Get_accumulate_local_atomic_async(const void *origin, void *result, void *target,
                                           MPIX_Aint count, MPIX_Datatype datatype, MPIX_Op op,
                                           void *stream);
int MPIX_Get_accumulate_local_atomic(const void *origin, void *result, void *target,
                                     MPIX_Aint count, MPIX_Datatype datatype, MPIX_Op op);

/* MPIX_Compare_and_swap_local as one device-scope compare-exchange, atomic as
 * above (also against the atomic accumulates on the same element).  The type
 * rule and the checks are MPIX_Compare_and_swap_local's; then the 16-byte
 * types are MPI_ERR_TYPE (no 128-bit atomic), a target not aligned to its size
 * or not device memory of the stream's device MPI_ERR_BUFFER.  origin, compare
 * and result need no alignment. */
int MPIX_Compare_and_swap_local_atomic_async(const void *origin, const void *compare,
                                             void *result, void *target, MPIX_Datatype datatype,
                                             void *stream);
int MPIX_Compare_and_swap_local_atomic(const void *origin, const void *compare, void *result,
                                       void *target, MPIX_Datatype datatype);

/* 1 exactly when the atomic entries take (op, datatype): the pair is legal, it
 * has a kernel, and the internal type's extent is 1, 2, 4 or 8 bytes; with
 * MPI_OP_NULL it asks about MPIX_Compare_and_swap_local_atomic (the type is
 * RMA-atomic and at most 8 bytes).  MPIX_EQUAL is 0.  No HIP call: query once
 * per window and (type, op), as MPIDI_OFI_query_acc_atomic_support does
 * (max_count == 0 <-> 0 here). */
int MPIX_Accumulate_atomic_is_supported(MPIX_Op op, MPIX_Datatype datatype);

/* Multi-input form: equivalent to `ninputs` MPIX_Reduce_local calls
 *   for k = 0 .. ninputs-1:  inoutbuf = inoutbuf OP inbufs[k]
 * in that order (same association, same bits) but done in one pass over
 * memory.  Used by reduce-scatter schedules whose received blocks arrive
 * together (pairwise, reduce_scatter_block_intra_pairwise.c:86-100).
 * 1 <= ninputs <= 16; device-accessible buffers; stream-ordered. */
int MPIX_Reduce_local_multi_async(const void *const *inbufs, int ninputs, void *inoutbuf,
                                  MPIX_Aint count, MPIX_Datatype datatype, MPIX_Op op,
                                  void *stream);

/* Tree form: outbuf = the pairwise tree fold of ninputs = 2^L slots
 * (2 <= ninputs <= 16), level by level m = 1, 2, 4, ...:
 *   slot s (bit m of s clear) = slot s OP slot s+m   (slot s is inout)
 * and outbuf = slot 0.  inbufs[0] must be given; a NULL slot s > 0 is absent:
 * at its level the partner passes through unchanged (the first level of the
 * reference's fold of a non-power-of-two world, where only the paired ranks
 * combine).  Holding the block of rank r ^ bitrev(s) in slot s,
 * this is the association recursive halving gives rank r's block
 * (reduce_scatter_block_intra_recursive_halving.c:164-229, P a power of
 * two), so a schedule that can read every peer's block computes the
 * reference's bits in one pass.  outbuf may be one of the slots exactly (in
 * place); no partial overlap.  REPLACE yields the last present slot, NO_OP
 * the first; MPIX_EQUAL is refused (MPI_ERR_OP).  Device-accessible buffers;
 * stream-ordered. */
int MPIX_Reduce_local_tree_async(const void *const *inbufs, int ninputs, void *outbuf,
                                 MPIX_Aint count, MPIX_Datatype datatype, MPIX_Op op,
                                 void *stream);

/* n <= 16 independent copies dsts[q] <- srcs[q] (bytes[q] each) in ONE
 * stream-ordered launch, all running at once -- the allgather step of a pull
 * schedule, whose P-1 sources sit behind P-1 different xGMI links.
 * Device-accessible, non-overlapping pairs; zero-byte entries are skipped. */
int MPIX_Copy_multi_async(const void *const *srcs, void *const *dsts, const MPIX_Aint *bytes,
                          int n, void *stream);

/* ---- peer memory for the fused pull + combine ----
 * The reference maps peer GPU buffers with hipIpc* in its shm/ipc path
 * (src/mpl/src/gpu/mpl_gpu_hip.c:174-204).  Here a rank exports the
 * allocation holding `devptr` (handle: MPIX_IPC_HANDLE_BYTES opaque bytes,
 * plus the byte offset of devptr inside it); peers open it and pass the
 * mapped addresses straight to MPIX_Reduce_local_multi_async, so the combine
 * kernel reads the peers' blocks over xGMI with no intermediate copy. */
#define MPIX_IPC_HANDLE_BYTES 64
int MPIX_Ipc_export(const void *devptr, void *handle_out, MPIX_Aint *offset_out);
int MPIX_Ipc_open(const void *handle, void **base_out);
int MPIX_Ipc_close(void *base);

/* ---- operands on two devices ----
 * 1 if kernels on `device` can dereference memory of `peer_device` (same
 * device, or peer access enabled -- by this call at the pair's first use,
 * once per process), else 0.  Replaces the all-pairs loop of the reference's
 * HIP init hook (yaksa/src/backend/hip/hooks/yaksuri_hip_init_hooks.c:164-181:
 * hipDeviceCanAccessPeer, hipDeviceEnablePeerAccess, "already enabled"
 * tolerated).  Every entry point settles its pairs itself: MPIX_Reduce_local
 * runs on inout's device and, without peer access, copies `in` over with
 * hipMemcpyPeerAsync; the stream-ordered entry points return MPI_ERR_BUFFER
 * for an operand the stream's device cannot reach.  Env MPIX_REDOP_PEER=stage
 * treats every pair of distinct devices as unreachable. */
int MPIX_Redop_peer_access(int device, int peer_device);

/* 1 if (op, datatype) goes to the GPU path, else 0 -- the contract of
 * MPIR_Typerep_reduce_is_supported (typerep_yaksa_pack.c:227-271), which
 * reduce_local.c:68 (count 0) and maint/gen_coll.py:546-547 (count of the
 * collective) consult.  0 when the path is disabled (env MPIX_REDOP_ENABLE=0,
 * as MPIR_CVAR_ENABLE_YAKSA_REDUCTION), when count > 0 and the packed size
 * count * size exceeds the threshold (env MPIX_REDOP_THRESHOLD bytes, default
 * -1 = no limit, as MPIR_CVAR_YAKSA_REDUCTION_THRESHOLD), or when no kernel
 * covers the pair.  When 0, a caller keeps its own CPU op table. */
int MPIX_Redop_is_supported(MPIX_Op op, MPIX_Aint count, MPIX_Datatype datatype);

/* 1 if a GPU kernel covers (op, datatype), whatever the knobs above say (the
 * collectives of libmpix_coll decline a pair only when this is 0, so
 * MPIX_REDOP_ENABLE=0 never turns them off). */
int MPIX_Redop_has_gpu_path(MPIX_Op op, MPIX_Datatype datatype);

/* The same predicate with the operands in view, for reduce_local.c's branch:
 * additionally 0 when BOTH buffers are host-resident and one operand holds
 * fewer bytes than the host floor of its memory kind (pageable: env
 * MPIX_REDOP_HOST_FLOOR, page-locked: MPIX_REDOP_PINNED_FLOOR), below which one
 * core's op_fns.c loop beats the round trip over PCIe (crossover measured by
 * bench.py, `host_crossover`).  A device-resident operand always answers as
 * MPIX_Redop_is_supported does. */
int MPIX_Redop_is_supported_buffers(MPIX_Op op, MPIX_Aint count, MPIX_Datatype datatype,
                                    const void *inbuf, const void *inoutbuf);

/* The predicate's knobs at run time (the env variables above set them at
 * first use): enable 0/1, threshold (<= 0: none), the two host floors
 * (<= 0: no floor). */
int MPIX_Redop_set_support(int enable, MPIX_Aint threshold_bytes, MPIX_Aint host_floor_bytes,
                           MPIX_Aint pinned_floor_bytes);
int MPIX_Redop_get_support(int *enable, MPIX_Aint *threshold_bytes, MPIX_Aint *host_floor_bytes,
                           MPIX_Aint *pinned_floor_bytes);

/* Binding-level and internal legality of (op, datatype): 1 legal, 0 not. */
int MPIX_Redop_op_dt_check(MPIX_Op op, MPIX_Datatype datatype);
int MPIX_Redop_internal_op_dt_check(MPIX_Op op, MPIX_Datatype datatype);

/* External builtin -> internal type (identity for internal / pair handles,
 * MPIX_DATATYPE_NULL (0x0c000000) for unknown builtins). */
MPIX_Datatype MPIX_Datatype_internal(MPIX_Datatype datatype);
/* Extent in bytes of one element (pair types include padding); 0 if unknown. */
MPIX_Aint MPIX_Datatype_extent(MPIX_Datatype datatype);
/* Size in bytes of one element's data (MPIR_Datatype_get_size_macro):
 * the extent, except for the padded pairs DOUBLE_INT / LONG_INT (12),
 * SHORT_INT (6) and LONG_DOUBLE_INT (20); 0 if unknown. */
MPIX_Aint MPIX_Datatype_size(MPIX_Datatype datatype);

/* Fortran .TRUE./.FALSE. used by LAND/LOR/LXOR on Fortran logicals
 * (mpii_fortlogical.h:15,28; defaults 1 / 0 as typeutil.c:502-510). */
int MPIX_Redop_set_fortran_booleans(int true_value, int false_value);

/* ---- per-op function table, MPIR_op_function signature (mpir_op.h:206) ----
 * Synchronous; same pointer rules as MPIX_Reduce_local.  Only pairs that
 * MPIX_Redop_is_supported() accepts may be passed: the op functions return
 * void like the reference's, and a call that fails (a pair no kernel covers,
 * e.g. MPI_MAX on MPIX_BFLOAT16, or a HIP error) prints the reason and abort()s, as
 * the reference's MPIR_Assert(0) does (op_fns.c:51-53).  With env
 * MPIX_REDOP_OPFN_ABORT=0 the failure is only recorded and can be read with
 * MPIX_Redop_last_error(). */
typedef void MPIX_op_function(void *invec, void *inoutvec, MPIX_Aint *len,
                              MPIX_Datatype *type);
extern MPIX_op_function *const MPIX_Op_table[16];
void MPIX_MAXF(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_MINF(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_SUM_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_PROD_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_LAND_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_BAND_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_LOR_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_BOR_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_LXOR_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_BXOR_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_MINLOC_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_MAXLOC_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_REPLACE_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
void MPIX_NO_OP_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);
/* MPIX_EQUAL (opequal.c:20-35): MPI_BYTE, 8-byte is_equal header + payload */
void MPIX_EQUAL_fn(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type);

int MPIX_Redop_last_error(void);
const char *MPIX_Redop_error_string(int code);

/* ---- several ready chunks in one launch (stream-ordered) ----
 * k independent combines inoutbufs[i][j] = OP(inoutbufs[i][j], inbufs[i][j]),
 * j < counts[i], i < k, of one datatype and op, issued as ONE kernel launch on
 * `stream`: the same bits as k MPIX_Reduce_local_async calls (each segment is
 * split into head / packets / tail exactly as a call of its own would be) at
 * the host cost of one launch (HIP's issue is ~2.5 us per launch,
 * profiles/r04_call_floor.json).  For the engines that find several vertices
 * ready at once -- gentran_utils.c:157-167 calls MPIR_Reduce_local per ready
 * reduce vertex, mpidu_sched.c:309-316 per reduce entry of a schedule round.
 * 1 <= k <= MPIX_BATCH_MAX, else MPI_ERR_ARG; no triple's target range may
 * overlap another triple's target or source range (MPI_ERR_BUFFER: the
 * segments run in no particular order); zero counts are skipped; every
 * operand must be reachable from the stream's device, as for
 * MPIX_Reduce_local_async.  All checks happen before any device work.
 * MPI_REPLACE / MPI_NO_OP / MPIX_EQUAL, operands that are not element-aligned
 * (for the 32-byte pair and complex types: not 16-byte aligned) and triples
 * with a page-locked host operand (read over PCIe by the capped, looping
 * zero-copy grid) are issued one launch per triple. */
#define MPIX_BATCH_MAX 64
int MPIX_Reduce_local_batch_async(const void *const *inbufs, void *const *inoutbufs,
                                  const MPIX_Aint *counts, int k, MPIX_Datatype datatype,
                                  MPIX_Op op, void *stream);

/* ---- launch geometry (performance knob, not semantics) ----
 * threads per block and a cap on the grid (0 = one tile per block, no
 * grid-stride loop).  The packets-per-thread unroll is a compile-time
 * constant (MPIX_REDOP_UNROLL).  Env MPIX_REDOP_BLOCK / MPIX_REDOP_MAXGRID
 * override the defaults at first use.  Kernels that read page-locked host
 * memory over PCIe (zero-copy) run at most 16384 threads' worth of looping
 * blocks (256 at the default 64 threads) unless max_grid is smaller, so loads
 * and stores share the link both ways; env MPIX_REDOP_ZC_GRID sets that cap
 * in blocks (0: none).  Defaults: 64-thread blocks, one 16-byte packet per
 * lane per operand. */
int MPIX_Redop_set_launch(int block_threads, int max_grid);
int MPIX_Redop_get_launch(int *block_threads, int *unroll, int *max_grid);

/* ---- store policy of the contiguous kernel (performance knob, not semantics) ----
 * Blocks of a contiguous launch that run on an XCD whose bit is set in
 * xcd_mask (HW_REG_XCC_ID, bits 0-7), blocks b with b % every == phase
 * (every > 0), and the last tail_blocks blocks store their result
 * write-through (the line leaves the XCD's L2 at once) instead of
 * non-temporally (the line stays in L2, dirty, until evicted or written back
 * at the end of the kernel).  Same bits either way.  Default (xcd_mask -1):
 * 0x88 (two XCDs of eight write through: 8-9 % faster at 1 GiB) when every
 * visible device has 8 XCDs, else 0, settled at the first kernel launch --
 * get_store_policy reports -1 until then, the settled mask after; set -1 to
 * return to it.  every = tail_blocks = 0.  Env MPIX_REDOP_WT_XCD /
 * MPIX_REDOP_WT_EVERY / MPIX_REDOP_WT_PHASE / MPIX_REDOP_WT_TAIL override
 * the defaults at first use.  Neither call, nor any support predicate or
 * other knob, makes a HIP call. */
int MPIX_Redop_set_store_policy(int xcd_mask, int every, int phase, int tail_blocks);
int MPIX_Redop_get_store_policy(int *xcd_mask, int *every, int *phase, int *tail_blocks);

/* The synchronous entry's own XCD mask (MPIX_Reduce_local on device or
 * page-locked operands: the MPIR_Reduce_local drop-in, whose kernels start
 * from an idle GPU call after call).  Default (-1): the mask set with
 * MPIX_Redop_set_store_policy / MPIX_REDOP_WT_XCD if any, else 0x22 on
 * 8-XCD devices (XCDs 1 and 5: the faster synchronous call,
 * profiles/r05_sync_xcd_masks.json), 0 otherwise; env MPIX_REDOP_WT_XCD_SYNC
 * at first use.  get reports the mask the next synchronous launch uses (-1
 * while the default is unsettled).  No HIP call. */
int MPIX_Redop_set_sync_store_policy(int xcd_mask);
int MPIX_Redop_get_sync_store_policy(int *xcd_mask);

/* Kernel timing of the synchronous entry, for measurement (bench.py's
 * roofline figure): the calling thread's next ncalls synchronous calls on
 * `device` (MPIX_Reduce_local on device or page-locked operands) record a HIP
 * event pair around their launch on the library's stream -- the combine as the
 * call runs it, nothing else changed.  ncalls = 0 stops; at most 65536.
 * _read waits for the recorded pairs, stores up to cap durations (ms, call
 * order) in ms[], their number in *got, and stops the recording.  No
 * counterpart in MPICH (a tool interface, like the MPIX_Redop_set_* knobs). */
int MPIX_Redop_sync_timing(int device, int ncalls);
int MPIX_Redop_sync_timing_read(int device, float *ms, int cap, int *got);

/* ---- large pageable host operands (performance knob) ----
 * threads > 0: pageable operands of at least 2 * chunk_bytes go through that many
 * host threads (the caller is one of them).  Default form, "wave": the
 * threads copy one chunk at a time into a page-locked buffer together (each
 * a slice), and ONE zero-copy kernel combines that chunk while they copy the
 * next one in and the previous result out; three chunk buffers rotate, and
 * the chunk sizes ramp up and down at both ends (short pipeline fill).  Env
 * MPIX_REDOP_PAGEABLE_MODE=worker selects the round-2 form instead: each
 * thread copies, combines and copies back chunks of its own (operands of at
 * least 2 * threads * chunk_bytes; env MPIX_REDOP_PAGEABLE_DB=1 gives every
 * thread two buffers).  Smaller operands, and all of them with threads = 0,
 * are staged through device scratch with hipMemcpyAsync.  Same bits every
 * way.  Defaults 8 threads x 64 MiB (env MPIX_REDOP_PAGEABLE_THREADS /
 * MPIX_REDOP_PAGEABLE_CHUNK at first use); threads 0..16, chunk 64 KiB..256
 * MiB.  The buffers are one set per device for the whole process (wave: 3 x
 * 2 x chunk of page-locked memory, 384 MiB at the defaults; worker: threads
 * x 2 x chunk, twice that with two buffers), freed by MPIX_Redop_finalize; a
 * call that finds the set in use by another thread stages its operands
 * instead.  Copies into the page-locked buffers use non-temporal stores (env
 * MPIX_REDOP_PAGEABLE_NT=0: memcpy), and env MPIX_REDOP_PAGEABLE_AFFINITY=gpu
 * pins the threads to the CPUs of the GPU's NUMA node (or to an explicit
 * cpulist such as "64-127"; default none). */
int MPIX_Redop_set_pageable(int threads, MPIX_Aint chunk_bytes);
int MPIX_Redop_get_pageable(int *threads, MPIX_Aint *chunk_bytes);

/* Build identification: the gfx target the code object was compiled for. */
const char *MPIX_Redop_build_info(void);

#define MPIX_DATATYPE_NULL ((MPIX_Datatype)0x0c000000)

#ifdef __cplusplus
}
#endif
#endif /* MPIX_REDOP_H_INCLUDED */
