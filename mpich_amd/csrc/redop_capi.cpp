// redop_capi.cpp -- the C-ABI of libmpix_redop.so (include/mpix_redop.h).
//
// Host side of the drop-in for MPIR_Reduce_local
// (src/mpi/coll/reduce_local/reduce_local.c:53-96): handle decoding,
// (op, datatype) legality, pointer classification, the per-thread stream,
// host-buffer staging, and the dispatch to the gfx950 kernels instantiated in
// inst_{int,fp,pair}.hip and inst_getacc_*.hip.  There is no CPU compute path
// here: a combination the GPU path does not cover returns MPIX_REDOP_ERR_TYPE and
// MPIX_Redop_is_supported() says so, so the caller keeps its own op table
// for it (exactly how reduce_local.c:66-76 falls back when yaksa declines).
#include <hip/hip_runtime_api.h>
#include <immintrin.h>

#include <ctype.h>
#include <limits.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <string>
#include <mutex>
#include <utility>
#include <vector>

#include "mpix_redop.h"
#include "redop_dispatch.h"
#include "redop_fixup.h"
#include "redop_hostpath.h"
#include "redop_runs.h"

using mpix::Entry;
using mpix::LaunchCfg;
using mpix::Params;

namespace {

// ---------------------------------------------------------------- handles
// Builtin index -> internal type (raw, index bits clear) and the binding
// group used by MPIR_op_dt_check.  LP64 x86-64 with Fortran: INTEGER, REAL,
// LOGICAL 4 bytes; DOUBLE PRECISION 8; long double 16 (x87 80-bit); bool 1.
// Source: src/mpi/datatype/typeutil.c:29-109 resolved by configure.ac:3446-3609.
enum Group { GN = 0, GCI, GFI, GFP, GLOG, GCPX, GBYTE, GMULTI };

struct Builtin {
    uint32_t internal;
    uint8_t group;
};

constexpr uint32_t I8 = 0x4c810100u, I16 = 0x4c810200u, I32 = 0x4c810400u, I64 = 0x4c810800u,
    I128 = 0x4c811000u, U8 = 0x4c820100u, U16 = 0x4c820200u, U32 = 0x4c820400u,
    U64 = 0x4c820800u, F16 = 0x4c830200u, F32 = 0x4c830400u, F64 = 0x4c830800u,
    F128 = 0x4c831000u, C16 = 0x4c840400u, C32 = 0x4c840800u, C64 = 0x4c841000u,
    C128 = 0x4c842000u, BF16 = 0x4c850200u, LD = 0x4c851000u, LDC = 0x4c862000u,
    L8 = 0x4c870100u, L16 = 0x4c870200u, L32 = 0x4c870400u, L64 = 0x4c870800u,
    L128 = 0x4c871000u, FX0 = 0x4c800000u, FX8 = 0x4c800100u, P2I32 = 0x4cc10800u,
    P2F32 = 0x4cc30800u, P2F64 = 0x4cc31000u;

struct BuiltinTable {
    Builtin e[0x4d];
    BuiltinTable() : e()
    {
        auto set = [this](int i, uint32_t t, uint8_t g) { e[i] = Builtin{t, g}; };
        set(0x01, I8, GCI);    set(0x02, U8, GCI);    set(0x03, I16, GCI);   set(0x04, U16, GCI);
        set(0x05, I32, GCI);   set(0x06, U32, GCI);   set(0x07, I64, GCI);   set(0x08, U64, GCI);
        set(0x09, I64, GCI);   set(0x0a, F32, GFP);   set(0x0b, F64, GFP);   set(0x0c, LD, GFP);
        set(0x0d, U8, GBYTE);  set(0x0e, I32, GN);    set(0x0f, FX8, GN);    set(0x10, FX0, GN);
        set(0x11, FX0, GN);    set(0x16, P2I32, GN);  set(0x18, I8, GCI);    set(0x19, U64, GCI);
        set(0x1a, I8, GN);     set(0x1b, I32, GFI);   set(0x1c, F32, GFP);   set(0x1d, L32, GLOG);
        set(0x1e, C32, GCPX);  set(0x1f, F64, GFP);   set(0x20, P2I32, GN);  set(0x21, P2F32, GN);
        set(0x22, C64, GCPX);  set(0x23, P2F64, GN);  set(0x26, F16, GFP);   set(0x27, F32, GFP);
        set(0x28, C32, GCPX);  set(0x29, F64, GFP);   set(0x2a, C64, GCPX);  set(0x2b, F128, GFP);
        set(0x2c, C128, GCPX); set(0x2d, I8, GFI);    set(0x2e, C16, GCPX);  set(0x2f, I16, GFI);
        set(0x30, I32, GFI);   set(0x31, I64, GFI);   set(0x32, I128, GFI);  set(0x33, I8, GLOG);
        set(0x34, C32, GCPX);  set(0x35, C64, GCPX);  set(0x36, LDC, GCPX);  set(0x37, I8, GCI);
        set(0x38, I16, GCI);   set(0x39, I32, GCI);   set(0x3a, I64, GCI);   set(0x3b, U8, GCI);
        set(0x3c, U16, GCI);   set(0x3d, U32, GCI);   set(0x3e, U64, GCI);   set(0x3f, I8, GLOG);
        set(0x40, C32, GCPX);  set(0x41, C64, GCPX);  set(0x42, LDC, GCPX);  set(0x43, I64, GMULTI);
        set(0x44, I64, GMULTI); set(0x45, I64, GMULTI); set(0x46, F16, GFP); set(0x47, L8, GLOG);
        set(0x48, L16, GLOG);  set(0x49, L32, GLOG);  set(0x4a, L64, GLOG);  set(0x4b, L128, GLOG);
        set(0x4c, BF16, GFP);
    }
};
const BuiltinTable kBuiltins;

constexpr uint32_t kNull = 0x0c000000u;

inline bool is_builtin(uint32_t h) { return (h >> 30) == 1u; }
inline bool is_struct_pair(uint32_t h) { return (h & 0xffffff00u) == 0x8c000000u && (h & 0xff) < 5; }
inline bool is_builtin_op(uint32_t op) { return (op >> 24) == 0x58u; }
// The builtin ops that are no combiner, by index (op & 0xf), and MPI_OP_NULL.
constexpr uint32_t kOpReplace = 13, kOpNoOp = 14, kOpEqual = 15, kOpNull = 0x18000000u;

// MPIR_DATATYPE_REPLACE_BUILTIN (mpir_datatype.h:169-176)
uint32_t to_internal(uint32_t dt)
{
    if (!is_builtin(dt) || (dt & 0x800000u))
        return dt;
    uint32_t idx = dt & 0xff;
    if (idx == 0 || idx >= 0x4d || kBuiltins.e[idx].internal == 0)
        return kNull;
    return kBuiltins.e[idx].internal | idx;
}

// element extent in bytes (pair padding included; pairtypes.c:15-21)
uint64_t extent_of(uint32_t it)
{
    if (is_struct_pair(it)) {
        static const uint64_t ext[5] = {8, 16, 16, 8, 32};
        return ext[it & 0xff];
    }
    if (!is_builtin(it) || it == kNull)
        return 0;
    return (it >> 8) & 0xff;
}

bool is_pairtype(uint32_t it)
{
    return is_struct_pair(it) || (is_builtin(it) && (it & 0x400000u));
}

int hip_err(hipError_t e);

// Type map of the struct pairs (pairtypes.c:24-80: a struct {value @0,
// int @idx_offset}, extent = sizeof the C struct).  DOUBLE_INT, LONG_INT,
// SHORT_INT and LONG_DOUBLE_INT have size < extent: their padding is not
// part of the type map, so a typemap copy (MPIR_Localcopy) leaves it alone
// and typerep_op_fallback treats them as "pairtype" (typerep_op.c:88).
struct PairMap {
    uint32_t value_bytes, loc_off;
};
bool padded_pair(uint32_t it, PairMap *pm)
{
    static const PairMap m[5] = {{4, 4}, {8, 8}, {8, 8}, {2, 4}, {16, 16}};
    if (!is_struct_pair(it) || (it & 0xff) == 0)
        return false;
    *pm = m[it & 0xff];
    return true;
}

// MPIR_Datatype_get_size_macro: bytes of data in one element
uint64_t size_of(uint32_t it)
{
    PairMap pm;
    if (padded_pair(it, &pm))
        return pm.value_bytes + 4;
    return extent_of(it);
}

// MPI_REPLACE (op_fns.c:445-457) = MPIR_Localcopy: `rows` elements at the
// given pitches.  Contiguous types copy whole extents; padded pairs copy the
// value and the int of each element (two pitched copies), so inout keeps its
// padding bytes exactly as the typemap copy does.
int replace_rows(void *dst, size_t dpitch, const void *src, size_t spitch, uint64_t rows,
                 uint32_t it, uint64_t ext, hipStream_t s)
{
    if (rows == 0)
        return MPIX_REDOP_SUCCESS;
    PairMap pm;
    if (!padded_pair(it, &pm)) {
        if (dpitch == ext && spitch == ext)
            return hip_err(hipMemcpyAsync(dst, src, rows * ext, hipMemcpyDeviceToDevice, s));
        return hip_err(hipMemcpy2DAsync(dst, dpitch, src, spitch, ext, rows,
                                        hipMemcpyDeviceToDevice, s));
    }
    int rc = hip_err(hipMemcpy2DAsync(dst, dpitch, src, spitch, pm.value_bytes, rows,
                                      hipMemcpyDeviceToDevice, s));
    if (rc == MPIX_REDOP_SUCCESS)
        rc = hip_err(hipMemcpy2DAsync((char *) dst + pm.loc_off, dpitch,
                                      (const char *) src + pm.loc_off, spitch, 4, rows,
                                      hipMemcpyDeviceToDevice, s));
    return rc;
}

// Type-map copy (MPIR_Localcopy) of `count` blocks of `bl` elements between
// two buffers whose blocks start every dp / sp elements.
int copy_blocks(void *dst, uint64_t dp, const void *src, uint64_t sp, uint64_t count,
                       uint64_t bl, uint32_t it, uint64_t ext, hipStream_t s)
{
    if (dp == bl && sp == bl)
        return replace_rows(dst, ext, src, ext, count * bl, it, ext, s);
    PairMap pm;
    if (!padded_pair(it, &pm))
        return hip_err(hipMemcpy2DAsync(dst, dp * ext, src, sp * ext, bl * ext, count,
                                        hipMemcpyDeviceToDevice, s));
    int rc = MPIX_REDOP_SUCCESS;
    if (bl <= count) {      // column k of every block
        for (uint64_t k = 0; k < bl && rc == MPIX_REDOP_SUCCESS; ++k)
            rc = replace_rows((char *) dst + k * ext, dp * ext, (const char *) src + k * ext,
                              sp * ext, count, it, ext, s);
    } else {                // block by block
        for (uint64_t b = 0; b < count && rc == MPIX_REDOP_SUCCESS; ++b)
            rc = replace_rows((char *) dst + b * dp * ext, ext, (const char *) src + b * sp * ext,
                              ext, bl, it, ext, s);
    }
    return rc;
}

// the signed and the unsigned integers among the internal types' kinds (it & 0x0f0000u)
inline bool integer_kind(uint32_t kind) { return kind == 0x010000u || kind == 0x020000u; }

// MPIR_Internal_op_dt_check (mpir_datatype.h:870-933)
bool internal_ok(uint32_t op, uint32_t it)
{
    if (!is_builtin_op(op))
        return false;
    uint32_t opi = op & 0xf;
    if (opi == 11 || opi == 12)
        return is_pairtype(it);
    if (opi >= kOpReplace)
        return true;
    if (!is_builtin(it) || !(it & 0x800000u) || (it & 0x400000u))
        return false;
    uint32_t kind = it & 0x0f0000u;
    switch (opi) {
        case 1: case 2:
            return integer_kind(kind) || kind == 0x030000u || kind == 0x050000u;
        case 3: case 4:
            return kind >= 0x010000u && kind <= 0x060000u;
        case 5: case 7: case 9:
            return integer_kind(kind) || kind == 0x070000u;
        case 6: case 8: case 10:
            return integer_kind(kind);
        default:
            return false;
    }
}

// MPIR_op_dt_check (mpir_datatype.h:780-868), builtin datatypes
bool binding_ok(uint32_t op, uint32_t dt)
{
    if (!is_builtin_op(op))
        return false;
    uint32_t opi = op & 0xf;
    if (opi == 11 || opi == 12)
        return is_pairtype(to_internal(dt));
    if (opi >= kOpReplace)
        return true;
    if (!is_builtin(dt))
        return false;
    if (dt & 0x800000u)
        return internal_ok(op, dt);
    uint32_t idx = dt & 0xff;
    if (idx == 0 || idx >= 0x4d || kBuiltins.e[idx].internal == 0)
        return false;
    uint8_t g = kBuiltins.e[idx].group;
    switch (opi) {
        case 1: case 2: return g == GCI || g == GFI || g == GFP || g == GMULTI;
        case 3: case 4: return g == GCI || g == GFI || g == GFP || g == GCPX || g == GMULTI;
        case 5: case 7: case 9: return g == GCI || g == GLOG || g == GMULTI;
        case 6: case 8: case 10: return g == GCI || g == GFI || g == GBYTE || g == GMULTI;
        default: return false;
    }
}

extern "C" const char *mpix_build_info(void);

// One family's entry of (op index, internal type): its fp, int and pair
// tables in turn.
template <class E>
const E *entry_of(const E *(*fp)(int, int), const E *(*in)(int, int), const E *(*pair)(int, int),
                  uint32_t opi, uint32_t it)
{
    const int raw = (int) (is_struct_pair(it) ? it : (it & 0xffffff00u));
    const E *e = fp(raw, (int) opi);
    if (!e)
        e = in(raw, (int) opi);
    if (!e)
        e = pair(raw, (int) opi);
    return e;
}

const Entry *gpu_entry(uint32_t opi, uint32_t it)
{
    return entry_of(mpix::lookup_fp, mpix::lookup_int, mpix::lookup_pair, opi, it);
}

// the fused get-accumulate's launchers of the same pair
const mpix::GetaccEntry *getacc_entry(uint32_t opi, uint32_t it)
{
    return entry_of(mpix::lookup_getacc_fp, mpix::lookup_getacc_int, mpix::lookup_getacc_pair, opi,
                    it);
}

// ... of its iov-target form
const mpix::GetaccIovEntry *getacc_iov_entry(uint32_t opi, uint32_t it)
{
    return entry_of(mpix::lookup_getacc_iov_fp, mpix::lookup_getacc_iov_int,
                    mpix::lookup_getacc_iov_pair, opi, it);
}

// ... and of the committed plans
const mpix::PlanEntry *plan_entry(uint32_t opi, uint32_t it)
{
    return entry_of(mpix::lookup_plan_fp, mpix::lookup_plan_int, mpix::lookup_plan_pair, opi, it);
}

// ... and of the typed entries (a datatype on every side)
const mpix::TypedEntry *typed_entry(uint32_t opi, uint32_t it)
{
    return entry_of(mpix::lookup_typed_fp, mpix::lookup_typed_int, mpix::lookup_typed_pair, opi,
                    it);
}

// ---------------------------------------------------------------- state
std::atomic<long long> g_ftrue{1}, g_ffalse{0};
// One-wave (64-thread) blocks of one packet per lane (round 5): kernel-trace
// durations of the synchronous 1 GiB fp32 SUM call 478 -> 460 us against
// 256-thread blocks, 448.7 against 480.6 us back to back; config-3 rows
// +3.3 % (median), the multi-input fold +4-8 % (tools/contig_u_probe.hip,
// tools/gpu_env_ab.sh, profiles/r05_block64_ab.json).
std::atomic<int> g_block{64}, g_max_grid{0};
// Grid cap of kernels reading page-locked host memory over PCIe (zero-copy):
// with one tile per block every block loads its whole tile (host to device)
// before it stores (device to host), and a grid of a few hundred blocks is
// one round, so the two link directions take turns.  Looping blocks keep
// both busy: with 4 packets per lane 32 blocks of 256 took 4 MiB 235 -> 186 us,
// 16 MiB 780 -> 655 us, 1 GiB 39.2 -> 38.1 ms (profiles/r04_pinned_grid.json);
// with one packet per lane (round 5) twice the lanes hold the same bytes in
// flight -- 64 blocks of 256: 1 MiB 69 -> 55 us, 4 MiB 238 -> 182 us, 16 MiB
// 769 -> 655 us, 256 MiB 10.1 -> 9.4 ms, where 32 gave 59 / 197 / 682 us /
// 9.8 ms (tools/pinned_grid.py, profiles/r05_pinned_grid.json).  The default
// cap is that many lanes (kZcLanes) in blocks of the current size;
// MPIX_REDOP_ZC_GRID sets it in blocks (0: uncapped).
constexpr int kZcLanes = 64 * 256;
constexpr int kZcAuto = -1;
std::atomic<int> g_zc_grid{kZcAuto};
// Store policy of the contiguous and multi-input kernels and the two-slot tree
// (MPIX_Redop_set_store_policy): the blocks running on the XCDs of g_wt_xcd
// store write-through (sc0 sc1), the others non-temporally.  Two XCDs of eight
// writing through make the 1 GiB fp32 SUM kernel 8-9 % faster at every operand
// placement tried, and every config-3 row 1-10 % faster (median 8 %); one XCD
// gains 4 %, three or four XCDs lose 1-5 %, all eight lose 3 %
// (profiles/r03_wt_probe_xcd.json, r03_wt_types_xcd88.json,
// r03_wt_sync_sweeps.txt).  Default: XCDs 3 and 7 on devices of 8 XCDs (SPX),
// off otherwise.  g_wt_every / g_wt_phase / g_wt_tail select blocks by index
// instead (the probes' forms).
// g_wt_xcd = kWtAuto until the first launch settles the default (resolve_wt,
// the only HIP query of the knobs: reading or setting them, and the support
// predicates, never start the HIP runtime).
constexpr int kWtAuto = -1;
std::atomic<int> g_wt_tail{0}, g_wt_every{0}, g_wt_phase{0}, g_wt_xcd{kWtAuto};
// The synchronous entry's own mask (MPIX_Redop_set_sync_store_policy, env
// MPIX_REDOP_WT_XCD_SYNC): MPIX_Reduce_local -- the MPIR_Reduce_local drop-in
// -- is timed by its callers call by call, each kernel starting from an idle
// GPU, and there XCDs 1 and 5 writing through (0x22) beat XCDs 3 and 7 (0x88)
// by 1.7-3.2 % per call on three boxes although the kernel alone is 2 %
// slower with it (profiles/r05_sync_xcd_masks.json).  The
// stream-ordered entries, whose kernels run back to back, keep g_wt_xcd.
// kWtAuto: an explicit g_wt_xcd if one was set, else the sync default.
std::atomic<int> g_wt_xcd_sync{kWtAuto};
std::once_flag g_wt_once;
// completion wait of the synchronous calls: 0 block (hipStreamSynchronize),
// 1 spin on an event, 2 spin on a pinned host word that a one-workgroup
// contiguous kernel stores itself and the stream writes after any other
// kernel (hipStreamWriteValue32; default), 3 the same word always written by
// the stream (10.1 vs 13.2 us for a 1-element call against the event,
// profiles/r01_lat_probe.txt) -- MPIX_REDOP_SYNC=block|event|flag|stream
std::atomic<int> g_sync{2};
std::atomic<bool> g_zero_copy{true}; // MPIX_REDOP_PINNED=stage stages pinned host memory too
std::once_flag g_env_once;
size_t g_stage_chunk = (size_t) 64 << 20;
// pageable operands up to this many bytes are copied (host memcpy) into a
// pinned bounce buffer the kernel reads and writes over PCIe, instead of three
// pageable hipMemcpy calls (each a driver-side bounce of its own);
// MPIX_REDOP_BOUNCE_BYTES, 0 disables
size_t g_bounce_bytes = (size_t) 1 << 20;
// large pageable operands (at least two chunks in the wave form below, two
// chunks per worker in the worker form): this many host threads copy chunks
// of g_pipe_chunk bytes into pinned buffers that zero-copy kernels combine
// (MPIX_REDOP_PAGEABLE_THREADS, 0 = always stream the chunks through device
// scratch with hipMemcpyAsync; MPIX_REDOP_PAGEABLE_CHUNK).  Wave form, 8 x
// 64 MiB: 1 GiB in 45-46 ms, 0.88 x the pinned zero-copy call
// (profiles/r03_pageable_wave_ramp.jsonl)
std::atomic<int> g_pipe_threads{8};
std::atomic<size_t> g_pipe_chunk{(size_t) 64 << 20};
// Worker form only: with MPIX_REDOP_PAGEABLE_DB=1 each worker keeps two slots
// and copies chunk k + W into one while the kernel of chunk k reads the other
// (default one slot: measured no faster, twice the pinned memory,
// profiles/r03_pageable_sweep.jsonl).  Both forms: the workers can be pinned
// to the CPUs of the GPU's own NUMA node (MPIX_REDOP_PAGEABLE_AFFINITY=gpu, or
// an explicit cpulist such as "64-127"; default "none" leaves them where the
// scheduler puts them -- pinning measured no faster either)
std::atomic<bool> g_pipe_db{false};
std::string g_pipe_affinity = "none";
// Pageable form (MPIX_REDOP_PAGEABLE_MODE): "wave" (default) -- all workers
// copy the same chunk in together (each a slice), ONE zero-copy kernel per
// chunk runs while they copy the next one in and the one before out, three
// pinned chunk buffers in rotation, chunk sizes ramped at both ends.  A
// zero-copy kernel pays a ramp of ~0.16 ms however large
// (profiles/r03_pinned_chunks.json), so large chunks win, and the ramped ends
// keep the pipeline fill short: 1 GiB in 45-46 ms at 8 x 64 MiB against
// 53 ms for the worker form (profiles/r03_pageable_wave_ramp.jsonl).
// "worker": each worker copies, combines and copies back chunks of its own.
std::atomic<int> g_pipe_wave{1};
// Support-predicate knobs, the pattern of MPIR_CVAR_ENABLE_YAKSA_REDUCTION and
// MPIR_CVAR_YAKSA_REDUCTION_THRESHOLD (typerep_yaksa_pack.c:44-64,229-240):
// MPIX_REDOP_ENABLE=0 makes every predicate answer 0 (the caller keeps its CPU
// op table); MPIX_REDOP_THRESHOLD > 0 declines calls whose packed size
// (count * type size) exceeds it (default -1, no limit).  The pointer-aware
// predicate also declines operands that are BOTH host-resident below a floor
// (MPIX_REDOP_HOST_FLOOR for pageable memory, MPIX_REDOP_PINNED_FLOOR for
// page-locked memory, bytes per operand): there one core's op_fns.c loop beats
// the PCIe round trip (crossover measured by bench.py's host_crossover leg).
std::atomic<bool> g_enable{true};
std::atomic<long long> g_threshold{-1};
// defaults from the crossover on MI355X + EPYC 9575F boxes, including the
// driver's (BENCH_r03 host_crossover, profiles/r04_pageable_swing.json): one
// core matches the pageable path up to 64 MiB per operand (the staged form at
// 1.00-1.05 x its time) and loses to it from 128 MiB on (0.4-0.8 x).  The
// page-locked zero-copy call lost to one core at 4 MiB (236 vs 216 us on the
// driver's box) until its kernel was capped to looping blocks (g_zc_grid):
// 169 vs 219 us at 4 MiB, even at 1 MiB (profiles/r04_bench_n1_zc.json).
// Below the floors MPICH keeps its op_fns.c loop.
std::atomic<long long> g_host_floor{(long long) 128 << 20};
std::atomic<long long> g_pinned_floor{(long long) 4 << 20};
// MPIX_Op_table entries return void, like MPIR_op_function: a call the GPU
// path declines aborts by default, as op_fns.c's MPIR_Assert(0) does
// (op_fns.c:51-53); MPIX_REDOP_OPFN_ABORT=0 only records the error
// (MPIX_Redop_last_error)
std::atomic<bool> g_opfn_abort{true};

void read_env()
{
    if (const char *s = getenv("MPIX_REDOP_BLOCK")) {
        int b = atoi(s);
        if (b >= 64 && b <= 1024 && b % 64 == 0)
            g_block = b;
    }
    if (const char *s = getenv("MPIX_REDOP_WT_TAIL"))
        g_wt_tail = atoi(s) > 0 ? atoi(s) : 0;
    if (const char *s = getenv("MPIX_REDOP_WT_EVERY"))
        g_wt_every = atoi(s) > 0 ? atoi(s) : 0;
    if (const char *s = getenv("MPIX_REDOP_WT_PHASE"))
        g_wt_phase = atoi(s) > 0 ? atoi(s) : 0;
    if (g_wt_every > 0)
        g_wt_phase = g_wt_phase % g_wt_every;
    if (const char *s = getenv("MPIX_REDOP_WT_XCD"))
        g_wt_xcd = (int) (strtol(s, nullptr, 0) & 0xff);
    if (const char *s = getenv("MPIX_REDOP_WT_XCD_SYNC"))
        g_wt_xcd_sync = (int) (strtol(s, nullptr, 0) & 0xff);
    if (const char *s = getenv("MPIX_REDOP_MAXGRID"))
        g_max_grid = atoi(s) > 0 ? atoi(s) : 0;
    if (const char *s = getenv("MPIX_REDOP_ZC_GRID"))
        g_zc_grid = atoi(s) > 0 ? atoi(s) : 0;
    if (const char *s = getenv("MPIX_REDOP_SYNC"))
        g_sync = strcmp(s, "block") == 0 ? 0
               : strcmp(s, "flag") == 0  ? 2
               : strcmp(s, "stream") == 0 ? 3
                                          : 1;
    if (const char *s = getenv("MPIX_REDOP_PINNED"))
        g_zero_copy = strcmp(s, "stage") != 0;
    if (const char *s = getenv("MPIX_REDOP_STAGE_CHUNK")) {
        long long c = atoll(s);
        if (c >= 4096)
            g_stage_chunk = (size_t) c;
    }
    if (const char *s = getenv("MPIX_REDOP_PAGEABLE_THREADS")) {
        int t = atoi(s);
        if (t >= 0 && t <= 16)
            g_pipe_threads = t;
    }
    if (const char *s = getenv("MPIX_REDOP_PAGEABLE_DB"))
        g_pipe_db = atoi(s) != 0;
    if (const char *s = getenv("MPIX_REDOP_PAGEABLE_MODE"))
        g_pipe_wave = strcmp(s, "worker") != 0;
    if (const char *s = getenv("MPIX_REDOP_PAGEABLE_AFFINITY"))
        g_pipe_affinity = s;
    if (const char *s = getenv("MPIX_REDOP_PAGEABLE_CHUNK")) {
        long long c = atoll(s);
        if (c >= 65536 && c <= (256ll << 20))
            g_pipe_chunk = (size_t) c;
    }
    if (const char *s = getenv("MPIX_REDOP_ENABLE"))
        g_enable = atoi(s) != 0;
    if (const char *s = getenv("MPIX_REDOP_THRESHOLD"))
        g_threshold = atoll(s);
    if (const char *s = getenv("MPIX_REDOP_HOST_FLOOR"))
        g_host_floor = atoll(s);
    if (const char *s = getenv("MPIX_REDOP_PINNED_FLOOR"))
        g_pinned_floor = atoll(s);
    if (const char *s = getenv("MPIX_REDOP_OPFN_ABORT"))
        g_opfn_abort = atoi(s) != 0;

    if (const char *s = getenv("MPIX_REDOP_BOUNCE_BYTES")) {
        long long c = atoll(s);
        if (c >= 0 && c <= (64ll << 20))
            g_bounce_bytes = (size_t) c;
    }
}

thread_local int t_last_error = 0;

constexpr int kMaxDev = 64;
constexpr int kSyncTimingMax = 1 << 16;    // calls one MPIX_Redop_sync_timing covers

// Page-locked host memory and its device mapping: the bounce buffer, each
// worker's slot and the wave's ring.
struct PinnedBuf {
    char *host = nullptr, *dev = nullptr;
    size_t bytes = 0;
    bool alloc(size_t n)
    {
        void *h = nullptr, *hd = nullptr;
        if (hipHostMalloc(&h, n, hipHostMallocDefault) != hipSuccess)
            return false;
        if (hipHostGetDevicePointer(&hd, h, 0) != hipSuccess) {
            (void) hipHostFree(h);
            return false;
        }
        host = (char *) h;
        dev = (char *) hd;
        bytes = n;
        return true;
    }
    void free()
    {
        if (host)
            (void) hipHostFree(host);
        *this = PinnedBuf();
    }
};

struct DevState {
    bool init = false;
    hipStream_t s[2] = {nullptr, nullptr};
    hipEvent_t done = nullptr;          // completion marker for the spin wait
    volatile uint32_t *flag = nullptr;  // pinned host word for MPIX_REDOP_SYNC=flag
    uint32_t *flag_ctr = nullptr;       // device word: workgroups done (Params::done_ctr)
    uint32_t seq = 0;
    void *scratch = nullptr;    // 2 slots x (in chunk + inout chunk)
    size_t scratch_bytes = 0;
    // iov run tables, two slots used in turn, so back-to-back iov calls only
    // wait for the call before the previous one
    struct IovSlot {
        int64_t *tab = nullptr;     // device copy of the run table
        int64_t *host = nullptr;    // its pinned host staging copy
        size_t cap = 0;             // capacity of both in int64 entries
        hipEvent_t done = nullptr;  // recorded after the launches that read it
    } iov[2];
    uint32_t iov_next = 0;
    PinnedBuf bounce;           // in half + inout half
    // MPIX_Redop_sync_timing: an event pair around the launch of each of the
    // next t_cap synchronous calls on s[0] (t_used recorded so far)
    std::vector<hipEvent_t> tev;
    int t_cap = 0, t_used = 0;
};

// Large pageable operands: one stream + pinned slot pair per host worker, ONE
// set per device for the whole process (not per calling thread), so the
// pinned footprint is workers x 2 x chunk (256 MiB at the defaults) per device
// however many MPI_THREAD_MULTIPLE threads call in.  A call that finds the set
// busy stages its operands instead (same kernel, same bits).
struct PipeSlot {
    hipStream_t s = nullptr;
    PinnedBuf buf;          // nbuf buffers of (in half + inout half), half bytes each
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};     // kernel of the chunk in buffer k done
};
struct PipeSet {
    std::mutex mu;
    PipeSlot slot[16];      // one or two buffers each
    PipeSlot ring;          // wave mode: 3 chunk buffers (in half + inout half each), one stream
    size_t half = 0;        // slot half size; slots [0, threads) hold buf.host != nullptr
    int nbuf = 0;           // buffers per worker (2: double-buffered)
    bool cpus_known = false;
    std::vector<int> cpus;  // worker CPUs (empty: no pinning)
};
PipeSet *g_pipes = new PipeSet[64];     // per device; never destroyed (finalize frees the memory)
// Per-thread device state (streams, flag word, scratch).  A thread that exits
// hands its array to a process-wide pool and the next new thread takes it over
// instead of creating streams of its own, so MPI_THREAD_MULTIPLE codes that
// spawn and join worker threads keep a bounded set of HIP streams.  The hand-off
// makes no HIP call (it may run at process exit); work still queued on the
// streams stays ordered ahead of the next owner's.  MPIX_Redop_finalize frees
// the caller's array and the pooled ones.
std::mutex g_pool_mu;
std::vector<DevState *> *g_pool = new std::vector<DevState *>();  // never destroyed
struct DevHolder {
    DevState *arr = nullptr;
    ~DevHolder()
    {
        if (arr) {
            std::lock_guard<std::mutex> l(g_pool_mu);
            g_pool->push_back(arr);
        }
    }
};
thread_local DevHolder t_dev;

int set_err(int e)
{
    t_last_error = e;
    return e;
}

int hip_err(hipError_t e)
{
    if (e == hipSuccess)
        return MPIX_REDOP_SUCCESS;
    if (getenv("MPIX_REDOP_VERBOSE"))
        fprintf(stderr, "mpix_redop: HIP error %d (%s)\n", (int) e, hipGetErrorString(e));
    return MPIX_REDOP_ERR_OTHER;
}

DevState *dev_state(int dev)
{
    if (dev < 0 || dev >= kMaxDev)
        return nullptr;
    if (!t_dev.arr) {
        std::lock_guard<std::mutex> l(g_pool_mu);
        if (!g_pool->empty()) {
            t_dev.arr = g_pool->back();
            g_pool->pop_back();
        } else {
            t_dev.arr = new DevState[kMaxDev];
        }
    }
    DevState &d = t_dev.arr[dev];
    if (!d.init) {
        for (int k = 0; k < 2; ++k)
            if (hipStreamCreateWithFlags(&d.s[k], hipStreamNonBlocking) != hipSuccess)
                return nullptr;
        if (hipEventCreateWithFlags(&d.done, hipEventDisableTiming) != hipSuccess)
            return nullptr;
        void *f = nullptr;
        if (hipHostMalloc(&f, 64, hipHostMallocCoherent) == hipSuccess) {
            d.flag = (volatile uint32_t *) f;
            *d.flag = 0;
            void *c = nullptr;
            if (hipMalloc(&c, 256) == hipSuccess) {
                // zeroed on the state's own stream and waited for: the
                // null-stream hipMemset is not ordered before kernels on the
                // non-blocking streams that read this counter
                if (hipMemsetAsync(c, 0, 256, d.s[0]) == hipSuccess &&
                    hipStreamSynchronize(d.s[0]) == hipSuccess)
                    d.flag_ctr = (uint32_t *) c;
                else
                    (void) hipFree(c);
            }
        }
        d.init = true;
    }
    return &d;
}

// The environment knobs, read once; no HIP call (CPU-only entry points --
// the support predicates, the knob getters and setters -- come through here).
void env()
{
    std::call_once(g_env_once, read_env);
}

// The default store policy, settled at the first launch that needs it: XCDs
// 3 and 7 write through when every visible device has 8 XCDs (SPX), else
// none.  While g_wt_xcd is kWtAuto (no MPIX_REDOP_WT_XCD, no explicit mask
// from MPIX_Redop_set_store_policy, or -1 set there) the launches use it.
std::atomic<int> g_wt_default{kWtAuto}, g_wt_sync_default{kWtAuto};
int wt_default(bool sync = false)
{
    std::call_once(g_wt_once, [] {
        int ndev = 0;
        bool spx = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
        for (int d = 0; spx && d < ndev; ++d) {
            int x = 0;
            spx = hipDeviceGetAttribute(&x, hipDeviceAttributeNumberOfXccs, d) == hipSuccess &&
                  x == 8;
        }
        (void) hipGetLastError();
        g_wt_default = spx ? 0x88 : 0;
        g_wt_sync_default = spx ? 0x22 : 0;
    });
    return sync ? g_wt_sync_default.load() : g_wt_default.load();
}

// Launch geometry and store policy of a kernel about to be enqueued (sync:
// for the synchronous entry, g_wt_xcd_sync).
LaunchCfg launch_cfg(bool zero_copy = false, bool sync = false)
{
    env();
    int wt = g_wt_xcd.load();
    if (sync) {
        const int ws = g_wt_xcd_sync.load();
        if (ws != kWtAuto)
            wt = ws;
        else if (wt == kWtAuto)
            wt = wt_default(true);
    }
    if (wt == kWtAuto)
        wt = wt_default();
    LaunchCfg c{g_block.load(), g_max_grid.load(), g_wt_tail.load(), g_wt_every.load(),
                g_wt_phase.load(), wt};
    if (!zero_copy)
        return c;
    // ... of one whose operand(s) include page-locked host memory (g_zc_grid)
    int z = g_zc_grid.load();
    if (z == kZcAuto)
        z = kZcLanes / (c.block > 0 ? c.block : 64);
    if (zero_copy && z > 0 && (c.max_grid <= 0 || c.max_grid > z))
        c.max_grid = z;
    return c;
}

Params params() { return Params{g_ftrue.load(), g_ffalse.load()}; }

// Spin until the pinned completion word holds `seq`.  The stream is queried
// every 4096 spins once 20 ms have passed (a query inside a short spin costs
// latency): an idle stream means the work and the word's store are done; a
// stream in an error state (a faulted kernel) ends the wait with that error
// instead of spinning forever.
int spin_on_flag(DevState *d, hipStream_t s, uint32_t seq)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 1; __atomic_load_n(d->flag, __ATOMIC_ACQUIRE) != seq; ++spins) {
        if ((spins & 0xfff) != 0 ||
            std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(20))
            continue;
        hipError_t q = hipStreamQuery(s);
        if (q == hipErrorNotReady)
            continue;
        if (q == hipSuccess)
            return MPIX_REDOP_SUCCESS;
        return hip_err(q);
    }
    return MPIX_REDOP_SUCCESS;
}

// Completion wait of the synchronous entry points.  MPI progress engines
// poll; a blocking hipStreamSynchronize costs wake-up latency per call, and an
// event query goes through the runtime's signal path, so by default the
// stream writes a sequence number into pinned host memory after the kernel and
// the caller spins on that word.
int wait_stream(DevState *d, hipStream_t s)
{
    int mode = g_sync.load();
    if (mode == 0)
        return hip_err(hipStreamSynchronize(s));
    hipError_t e;
    if ((mode == 2 || mode == 3) && d->flag) {
        uint32_t seq = ++d->seq;
        e = hipStreamWriteValue32(s, (void *) d->flag, seq, 0);
        if (e != hipSuccess)
            return hip_err(e);
        return spin_on_flag(d, s, seq);
    }
    e = hipEventRecord(d->done, s);
    if (e != hipSuccess)
        return hip_err(e);
    while ((e = hipEventQuery(d->done)) == hipErrorNotReady) {
    }
    return hip_err(e);
}

using Where = mpix::Place;

// Device / managed memory is used in place.  Pinned (page-locked, mapped)
// host memory is read and written by the kernel directly over PCIe
// ("zero-copy": one pass, both link directions busy at once) unless
// MPIX_REDOP_PINNED=stage; pageable host memory has to be staged.
Where classify(const void *p, int *dev, const void **devptr)
{
    hipPointerAttribute_t a;
    hipError_t e = hipPointerGetAttributes(&a, p);
    *devptr = p;
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return Where::Pageable;
    }
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) {
        *dev = a.device;
        return Where::Device;
    }
    if (a.type == hipMemoryTypeHost && a.devicePointer) {
        // devicePointer maps the start of the allocation containing p
        *devptr = (const char *) a.devicePointer + ((const char *) p - (const char *) a.hostPointer);
        return Where::Pinned;
    }
    return Where::Pageable;
}

bool ranges_overlap(const void *a, uint64_t na, const void *b, uint64_t nb)
{
    const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
    return x < y + nb && y < x + na;
}

bool overlaps(const void *a, const void *b, uint64_t bytes)
{
    return ranges_overlap(a, bytes, b, bytes);
}

// NULL or MPI_IN_PLACE
bool no_buffer(const void *p) { return !p || p == (const void *) -1; }

// Argument checks shared by every entry point: the binding-layer checks of
// MPI_Reduce_local (binding_c.py:2774-2783: op/datatype legality, buffer
// aliasing, no MPI_IN_PLACE) plus count < 0.  On success *it holds the
// internal type and *ext its extent.
int validate(const void *in, const void *io, MPIX_Aint count, uint32_t dt, uint32_t op,
             uint32_t *it, uint64_t *ext)
{
    if (count < 0)
        return MPIX_REDOP_ERR_COUNT;
    if (!is_builtin_op(op))
        return MPIX_REDOP_ERR_OP;
    *it = to_internal(dt);
    if (*it == kNull)
        return MPIX_REDOP_ERR_TYPE;
    *ext = extent_of(*it);
    if (*ext == 0)
        return MPIX_REDOP_ERR_TYPE;
    if (!internal_ok(op, *it))
        return MPIX_REDOP_ERR_OP;
    if (count == 0)
        return MPIX_REDOP_SUCCESS;
    // no buffer spans 2^56 bytes; beyond that count * extent could wrap
    if ((uint64_t) count > ((uint64_t) 1 << 56) / *ext)
        return MPIX_REDOP_ERR_COUNT;
    if (!in || !io || in == (const void *) -1 || io == (const void *) -1)
        return MPIX_REDOP_ERR_BUFFER;
    if (overlaps(in, io, (uint64_t) count * *ext))
        return MPIX_REDOP_ERR_BUFFER;
    return MPIX_REDOP_SUCCESS;
}

// The combine to run: validated arguments, both buffers device-accessible.
struct Combine {
    const void *in;
    void *io;
    uint64_t count;
    uint32_t it;        // internal type
    uint64_t ext;       // its extent
    uint32_t op;
};

// run_sync's enqueue on the library stream, with its store policy.  prm.done
// set: on success with *signalled set, prm.done_seq will be stored to it once
// the result is complete (prm.done_ctr: its workgroup counter).
int enqueue_sync(const Combine &c, hipStream_t s, bool zero_copy, bool sync, const Params &prm,
                 bool *signalled)
{
    *signalled = false;
    uint32_t opi = c.op & 0xf;
    if (opi == kOpNoOp)
        return MPIX_REDOP_SUCCESS;
    if (opi == kOpReplace)      // = MPIR_Localcopy (op_fns.c:445-457)
        return replace_rows(c.io, c.ext, c.in, c.ext, c.count, c.it, c.ext, s);
    if (opi == kOpEqual)        // MPI_BYTE only (opequal.c:22-23)
        return ((c.it & 0xffffff00u) == U8 && c.count >= 8)
            ? hip_err(mpix::launch_equal(c.in, c.io, c.count, s)) : MPIX_REDOP_ERR_TYPE;
    const Entry *e = gpu_entry(opi, c.it);
    if (!e)
        return MPIX_REDOP_ERR_TYPE;
    int rc = hip_err(e->contig(c.in, c.io, c.count, prm, launch_cfg(zero_copy, sync), s));
    *signalled = prm.done && rc == MPIX_REDOP_SUCCESS;
    return rc;
}

// Enqueue on a stream (zero_copy: an operand is page-locked host memory).
int enqueue(const Combine &c, hipStream_t s, bool zero_copy = false)
{
    bool signalled;
    return enqueue_sync(c, s, zero_copy, false, params(), &signalled);
}

// Synchronous combine of device-accessible operands on the library stream.
// With the default flag wait, the contiguous launcher signals completion
// itself (a kernel of at most kSignalMaxGrid workgroups stores the word,
// saving the end-of-kernel and stream-packet round trip:
// profiles/r01_sync_latency.txt); other ops and the other wait modes go
// through wait_stream.
int run_sync(DevState *d, const Combine &c, bool zero_copy = false)
{
    launch_cfg();       // environment read before g_sync is consulted
    // timed call (MPIX_Redop_sync_timing): the pair brackets the launch on
    // the state's stream, nothing else changes
    const int ti = d->t_used < d->t_cap ? d->t_used++ : -1;
    if (ti >= 0) {
        int rc = hip_err(hipEventRecord(d->tev[2 * ti], d->s[0]));
        if (rc)
            return rc;
    }
    struct Stop {
        DevState *d;
        int ti;
        ~Stop()
        {
            if (ti >= 0)
                (void) hipEventRecord(d->tev[2 * ti + 1], d->s[0]);
        }
    };
    Params prm = params();
    if (g_sync.load() == 2 && d->flag) {
        prm.done = (uint32_t *) d->flag;
        prm.done_ctr = d->flag_ctr;
        prm.done_seq = ++d->seq;
    }
    bool signalled = false;
    int rc;
    {
        Stop stop{d, ti};
        rc = enqueue_sync(c, d->s[0], zero_copy, true, prm, &signalled);
    }
    if (signalled)      // the kernel stores the word itself
        return spin_on_flag(d, d->s[0], prm.done_seq);
    int rc2 = wait_stream(d, d->s[0]);
    return rc ? rc : rc2;
}

// ------------------------------------------- host-resident operands
// The forms mpix::host_route picks from.  in_host / io_host: the form copies
// that operand itself; the other one is device-accessible as given.

// Device scratch of at least `need` bytes.  A smaller buffer is freed once
// both library streams are idle (work queued on them may still use it).
bool device_scratch(DevState *d, size_t need)
{
    if (d->scratch_bytes >= need)
        return true;
    if (d->scratch) {
        (void) hipStreamSynchronize(d->s[0]);
        (void) hipStreamSynchronize(d->s[1]);
        (void) hipFree(d->scratch);
    }
    d->scratch = nullptr;
    d->scratch_bytes = 0;
    if (hipMalloc(&d->scratch, need) != hipSuccess)
        return false;
    d->scratch_bytes = need;
    return true;
}

// Copy-in of an operand the kernel will read from `dst`: device memory of
// in_peer, which `dev` cannot reach (hipMemcpyPeerAsync), or host memory;
// neither: nothing, the operand is used in place.
int stage_in(void *dst, const void *src, size_t bytes, int dev, int in_peer, bool host,
             hipStream_t s)
{
    if (in_peer >= 0)
        return hip_err(hipMemcpyPeerAsync(dst, dev, src, in_peer, bytes, s));
    if (host)
        return hip_err(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    return MPIX_REDOP_SUCCESS;
}

// Elements [off, off + n) of c as a form's kernel sees them: an operand the
// form copied in its half of `buf` (in first), another in place.
Combine chunk_of(const Combine &c, uint64_t off, uint64_t n, bool in_copied, bool io_copied,
                 char *buf, size_t half)
{
    return Combine{in_copied ? (const void *) buf : (const char *) c.in + off * c.ext,
                   io_copied ? (void *) (buf + half) : (char *) c.io + off * c.ext,
                   n, c.it, c.ext, c.op};
}

// Host-resident operand(s): stream them through device scratch in chunks,
// alternating two streams so chunk k+1's copies overlap chunk k's kernel.
// in_peer >= 0: `in` is device memory of that device, which `dev` cannot reach
// (no peer access): it is streamed the same way with hipMemcpyPeerAsync.
int staged(DevState *d, const Combine &c, bool in_host, bool io_host, int dev, int in_peer)
{
    uint64_t chunk_elems = g_stage_chunk / c.ext;
    if (chunk_elems == 0)
        chunk_elems = 1;
    if (chunk_elems > c.count)
        chunk_elems = c.count;
    size_t slot_bytes = (size_t) (chunk_elems * c.ext + 255) & ~(size_t) 255;
    if (!device_scratch(d, 4 * slot_bytes))     // 2 slots x (in chunk + inout chunk)
        return MPIX_REDOP_ERR_OTHER;
    int rc = MPIX_REDOP_SUCCESS;
    for (uint64_t off = 0, k = 0; off < c.count && rc == MPIX_REDOP_SUCCESS;
         off += chunk_elems, ++k) {
        uint64_t n = (c.count - off < chunk_elems) ? c.count - off : chunk_elems;
        hipStream_t s = d->s[k & 1];
        char *slot = (char *) d->scratch + (k & 1) * 2 * slot_bytes;
        char *dst_io = (char *) c.io + off * c.ext;
        const Combine kc = chunk_of(c, off, n, in_host || in_peer >= 0, io_host, slot, slot_bytes);
        rc = stage_in(slot, (const char *) c.in + off * c.ext, n * c.ext, dev, in_peer, in_host, s);
        if (rc == MPIX_REDOP_SUCCESS)
            rc = stage_in(slot + slot_bytes, dst_io, n * c.ext, dev, -1, io_host, s);
        if (rc == MPIX_REDOP_SUCCESS)
            rc = enqueue(kc, s);
        if (rc == MPIX_REDOP_SUCCESS && io_host)
            rc = hip_err(hipMemcpyAsync(dst_io, kc.io, n * c.ext, hipMemcpyDeviceToHost, s));
    }
    int rc2 = wait_stream(d, d->s[0]);
    int rc3 = wait_stream(d, d->s[1]);
    return rc ? rc : (rc2 ? rc2 : rc3);
}

// MPIX_EQUAL with host-resident operand(s) too large for the bounce buffer:
// whole-buffer copies into device scratch, ONE k_equal launch, and the 8-byte
// is_equal header back (k_equal writes nothing else).  When the scratch
// cannot be had nothing has been touched and MPI_ERR_TYPE sends the caller to
// its own op table.
int equal_whole(DevState *d, const Combine &c, bool in_host, bool io_host, int dev, int in_peer)
{
    const size_t n = (size_t) c.count;      // MPI_BYTE
    const size_t half = (n + 255) & ~(size_t) 255;
    if (!device_scratch(d, 2 * half)) {
        (void) hipGetLastError();
        return MPIX_REDOP_ERR_TYPE;
    }
    hipStream_t s = d->s[0];
    char *scratch = (char *) d->scratch;
    const Combine kc = chunk_of(c, 0, n, in_host || in_peer >= 0, io_host, scratch, half);
    int rc = stage_in(scratch, c.in, n, dev, in_peer, in_host, s);
    if (rc == MPIX_REDOP_SUCCESS)
        rc = stage_in(scratch + half, c.io, n, dev, -1, io_host, s);
    if (rc == MPIX_REDOP_SUCCESS)
        rc = hip_err(mpix::launch_equal(kc.in, kc.io, n, s));
    if (rc == MPIX_REDOP_SUCCESS && io_host)
        rc = hip_err(hipMemcpyAsync(c.io, kc.io, 8, hipMemcpyDeviceToHost, s));
    int rc2 = wait_stream(d, s);
    return rc ? rc : rc2;
}

// Small pageable operand(s): memcpy into the pinned bounce buffer, one
// zero-copy kernel over it, memcpy the result back (a staged 1-element call
// costs ~42 us in three pageable hipMemcpy calls).
// Returns -1 when the bounce buffer cannot be had (caller stages).
int bounced(DevState *d, const Combine &c, bool in_host, bool io_host)
{
    size_t bytes = (size_t) (c.count * c.ext);
    if (!d->bounce.host && !d->bounce.alloc(2 * ((g_bounce_bytes + 255) & ~(size_t) 255)))
        return -1;
    const size_t half = d->bounce.bytes / 2;
    if (bytes > half)
        return -1;
    if (in_host)
        memcpy(d->bounce.host, c.in, bytes);
    if (io_host)
        memcpy(d->bounce.host + half, c.io, bytes);
    int rc = run_sync(d, chunk_of(c, 0, c.count, in_host, io_host, d->bounce.dev, half), true);
    if (rc == MPIX_REDOP_SUCCESS && io_host)
        memcpy(c.io, d->bounce.host + half, bytes);
    return rc;
}

// Copy into a pinned buffer the GPU is about to read over PCIe.  With plain
// stores the lines sit dirty in the CPU caches and every PCIe read of them is
// a snoop hit; non-temporal stores send them to DRAM (glibc's memcpy switches
// to those only above its own, L3-sized threshold, above our chunk size).
// MPIX_REDOP_PAGEABLE_NT=0 uses memcpy.
std::atomic<int> g_pipe_nt{-1};     // -1: not decided yet
__attribute__((target("avx2"))) static void copy_nt_avx2(char *dst, const char *src, size_t n)
{
    size_t head = (32 - ((uintptr_t) dst & 31)) & 31;
    if (head > n)
        head = n;
    memcpy(dst, src, head);
    dst += head;
    src += head;
    n -= head;
    size_t i = 0;
    for (; i + 128 <= n; i += 128) {
        __m256i a = _mm256_loadu_si256((const __m256i *) (src + i));
        __m256i b = _mm256_loadu_si256((const __m256i *) (src + i + 32));
        __m256i c = _mm256_loadu_si256((const __m256i *) (src + i + 64));
        __m256i d = _mm256_loadu_si256((const __m256i *) (src + i + 96));
        _mm256_stream_si256((__m256i *) (dst + i), a);
        _mm256_stream_si256((__m256i *) (dst + i + 32), b);
        _mm256_stream_si256((__m256i *) (dst + i + 64), c);
        _mm256_stream_si256((__m256i *) (dst + i + 96), d);
    }
    _mm_sfence();
    memcpy(dst + i, src + i, n - i);
}

void copy_to_pinned(char *dst, const char *src, size_t n)
{
    int nt = g_pipe_nt.load(std::memory_order_relaxed);
    if (nt < 0) {
        const char *e = getenv("MPIX_REDOP_PAGEABLE_NT");
        nt = (e ? atoi(e) != 0 : true) && __builtin_cpu_supports("avx2");
        g_pipe_nt.store(nt);
    }
    if (nt)
        copy_nt_avx2(dst, src, n);
    else
        memcpy(dst, src, n);
}

// The workers' CPUs, found once per device: those of the GPU's NUMA node
// (sysfs local_cpulist of its PCI function) or an explicit "a-b,c" list,
// intersected with this process's affinity; empty: no pinning
const std::vector<int> &worker_cpus(PipeSet &P, int dev)
{
    if (P.cpus_known)
        return P.cpus;
    P.cpus_known = true;
    std::vector<int> want;
    const std::string mode = g_pipe_affinity;
    if (mode == "gpu") {
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, sizeof bus, dev) == hipSuccess) {
            for (char *q = bus; *q; ++q)
                *q = (char) tolower(*q);
            std::string path = std::string("/sys/bus/pci/devices/") + bus + "/local_cpulist";
            if (FILE *f = fopen(path.c_str(), "r")) {
                char line[4096] = {0};
                if (fgets(line, sizeof line, f))
                    want = mpix::parse_cpulist(line);
                fclose(f);
            }
        }
        (void) hipGetLastError();
    } else if (mode != "none" && !mode.empty()) {
        want = mpix::parse_cpulist(mode.c_str());
    }
    cpu_set_t mine;
    if (want.empty() || sched_getaffinity(0, sizeof mine, &mine) != 0)
        return P.cpus;
    for (int c : want)
        if (c < CPU_SETSIZE && CPU_ISSET(c, &mine))
            P.cpus.push_back(c);
    return P.cpus;
}

// Large pageable operand(s): W host workers take chunks k = w, w + W, ...; per
// chunk a worker memcpys the pageable operand(s) into a pinned buffer of its
// own, runs one zero-copy kernel over the buffer's device mapping on its own
// stream (a pinned or device operand is used in place) and memcpys the result
// back once that kernel is done.  Double-buffered (default), a worker copies
// chunk k + W into its second buffer while chunk k's kernel runs.  The
// workers' host copies overlap each other's PCIe transfers, where
// hipMemcpyAsync from pageable memory serialises through the runtime's own
// bounce.  Each element is combined exactly once, by the same kernel, so the
// bits equal every other path's.  Returns -1 when the buffers cannot be had
// (caller stages).
int pipelined(const Combine &c, bool in_pg, bool io_pg, int dev, int nthreads)
{
    if (dev < 0 || dev >= kMaxDev)
        return -1;
    PipeSet &P = g_pipes[dev];
    std::unique_lock<std::mutex> busy(P.mu, std::try_to_lock);
    if (!busy.owns_lock())
        return -1;      // another thread is using the set: stage instead
    const size_t half = (g_pipe_chunk.load() + 255) & ~(size_t) 255;
    const int nbuf = g_pipe_db.load() ? 2 : 1;
    bool ready = P.half >= half && P.nbuf >= nbuf;
    for (int w = 0; ready && w < nthreads; ++w)
        ready = P.slot[w].buf.host != nullptr;
    if (!ready) {
        // (re)allocate every worker's buffers at the current chunk size
        for (PipeSlot &sl : P.slot) {
            if (sl.s)
                (void) hipStreamSynchronize(sl.s);
            sl.buf.free();
        }
        P.half = 0;
        P.nbuf = 0;
        for (int w = 0; w < nthreads; ++w) {
            PipeSlot &sl = P.slot[w];
            if (!sl.s && hipStreamCreateWithFlags(&sl.s, hipStreamNonBlocking) != hipSuccess)
                return -1;
            for (hipEvent_t *e = sl.ev; e < sl.ev + 2; ++e)
                if (!*e && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess)
                    return -1;
            if (!sl.buf.alloc(2 * half * (size_t) nbuf))
                return -1;
        }
        P.half = half;
        P.nbuf = nbuf;
    }
    const std::vector<int> &cpus = worker_cpus(P, dev);
    const uint64_t chunk = half / c.ext;
    if (chunk == 0)
        return -1;
    const uint64_t nchunks = (c.count + chunk - 1) / chunk;
    const int W = (int) std::min<uint64_t>((uint64_t) mpix::worker_count(nthreads), nchunks);
    mpix::FirstError err;
    // MPIX_REDOP_PIPE_TRACE=1: per chunk the host times (ns from the call's
    // start) of copy-in start / end, wait start / end, copy-out end, printed
    // as one JSON line to stderr (tools/pageable_probe.py reads them)
    mpix::StepTrace tr(nchunks);
    auto work = [&](int w) {
        PipeSlot &sl = P.slot[w];
        if (hipSetDevice(dev) != hipSuccess) {
            err.fail(MPIX_REDOP_ERR_OTHER);
            return;
        }
        char *hbuf[2] = {sl.buf.host, sl.buf.host + 2 * half};
        char *dbuf[2] = {sl.buf.dev, sl.buf.dev + 2 * half};
        // buffer b: copy chunk k's pageable operand(s) in, enqueue its kernel
        auto start = [&](uint64_t k, int b) -> int {
            const uint64_t off = k * chunk, n = std::min(chunk, c.count - off);
            const size_t bytes = (size_t) (n * c.ext);
            tr.mark(k, 0);
            if (in_pg)
                copy_to_pinned(hbuf[b], (const char *) c.in + off * c.ext, bytes);
            if (io_pg)
                copy_to_pinned(hbuf[b] + half, (char *) c.io + off * c.ext, bytes);
            tr.mark(k, 1);
            int rc = enqueue(chunk_of(c, off, n, in_pg, io_pg, dbuf[b], half), sl.s, true);
            return rc ? rc : hip_err(hipEventRecord(sl.ev[b], sl.s));
        };
        // chunk k's kernel done: its result back to the pageable inout
        auto finish = [&](uint64_t k, int b) -> int {
            tr.mark(k, 2);
            int rc = hip_err(hipEventSynchronize(sl.ev[b]));
            tr.mark(k, 3);
            if (rc == MPIX_REDOP_SUCCESS && io_pg) {
                const uint64_t off = k * chunk, n = std::min(chunk, c.count - off);
                memcpy((char *) c.io + off * c.ext, hbuf[b] + half, (size_t) (n * c.ext));
            }
            tr.mark(k, 4);
            return rc;
        };
        uint64_t k = (uint64_t) w;
        int b = 0, rc = k < nchunks ? start(k, b) : MPIX_REDOP_SUCCESS;
        for (; k < nchunks && rc == MPIX_REDOP_SUCCESS && err.ok(); k += (uint64_t) W) {
            const uint64_t kn = k + (uint64_t) W;
            if (nbuf == 2) {
                if (kn < nchunks)
                    rc = start(kn, b ^ 1);          // overlaps chunk k's kernel
                int rc2 = finish(k, b);
                rc = rc ? rc : rc2;
                b ^= 1;
            } else {
                rc = finish(k, b);
                if (rc == MPIX_REDOP_SUCCESS && kn < nchunks)
                    rc = start(kn, b);
            }
        }
        // no kernel of this worker is left reading its buffers when the call
        // returns, also when another worker's failure ended the loop early
        (void) hipStreamSynchronize(sl.s);
        err.fail(rc);
    };
    mpix::run_workers(W, cpus, work);
    if (tr.on) {
        fprintf(stderr, "{\"pipe_trace\": {\"W\": %d, \"chunk\": %zu, \"nbuf\": %d, ", W, half, nbuf);
        tr.print_ns(stderr);
    }
    return err.rc.load();
}

// Wave mode (see g_pipe_wave).  Step s: the caller launches the kernel of
// chunk s - 1 (its copy-in finished in step s - 1); every worker copies its
// slice of chunk s in and, once chunk s - 2's kernel is done, its slice of
// chunk s - 2 out; then all meet.  Buffer s % 3 held chunk s - 3, whose
// copy-out ended in step s - 1.  Same kernel per element, same bits.
// Returns -1 when the buffers cannot be had (caller stages).
int waved(const Combine &c, bool in_pg, bool io_pg, int dev, int nthreads)
{
    if (dev < 0 || dev >= kMaxDev)
        return -1;
    PipeSet &P = g_pipes[dev];
    std::unique_lock<std::mutex> busy(P.mu, std::try_to_lock);
    if (!busy.owns_lock())
        return -1;
    const size_t half = (g_pipe_chunk.load() + 255) & ~(size_t) 255;
    if (P.ring.buf.bytes < 6 * half) {
        if (P.ring.s)
            (void) hipStreamSynchronize(P.ring.s);
        P.ring.buf.free();
        if (!P.ring.s && hipStreamCreateWithFlags(&P.ring.s, hipStreamNonBlocking) != hipSuccess)
            return -1;
        for (hipEvent_t &e : P.ring.ev)
            if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
                return -1;
        if (!P.ring.buf.alloc(3 * 2 * half))
            return -1;
    }
    const std::vector<int> &cpus = worker_cpus(P, dev);
    const uint64_t chunk = half / c.ext;
    if (chunk == 0)
        return -1;
    // offsets and counts in elements, no chunk above a ring half
    const std::vector<mpix::Chunk> chunks = mpix::wave_chunks(c.count, chunk);
    const int64_t n = (int64_t) chunks.size();
    const int W = mpix::worker_count(nthreads);
    mpix::SpinBarrier bar(W);
    // MPIX_REDOP_PIPE_TRACE=1: per step and worker the host times (ns from the
    // call's start) at which the kernel launch (worker 0), the copy-in, the
    // wait for the kernel of chunk st - 2, its copy-out and the step's barrier
    // ended, and the CPU each worker started on -- one JSON line to stderr
    // (tools/pageable_swing.py reads it)
    mpix::StepTrace tr((size_t) (n + 2) * (size_t) W);
    std::vector<int> trace_cpu((size_t) (tr.on ? W : 0), -1);
    auto mark = [&](int64_t st, int w, int what) {
        tr.mark((size_t) st * (size_t) W + (size_t) w, what);
    };
    mpix::FirstError err;
    // chunk k, copied into buffer b, as its kernel sees it
    auto kernel_chunk = [&](int64_t k, int b) {
        return chunk_of(c, chunks[(size_t) k].off, chunks[(size_t) k].count, in_pg, io_pg,
                        P.ring.buf.dev + (size_t) b * 2 * half, half);
    };
    // worker w's slice of chunk k: its offset in the operands, in the chunk, its length
    auto part = [&](int64_t k, int w, size_t *at, size_t *lo, size_t *len) {
        *at = (size_t) (chunks[(size_t) k].off * c.ext);
        mpix::slice(w, W, (size_t) (chunks[(size_t) k].count * c.ext), lo, len);
    };
    auto work = [&](int w) {
        if (tr.on)
            trace_cpu[(size_t) w] = sched_getcpu();
        if (hipSetDevice(dev) != hipSuccess) {
            err.fail(MPIX_REDOP_ERR_OTHER);
        }
        for (int64_t st = 0; st <= n + 1; ++st) {
            if (w == 0 && st >= 1 && st - 1 < n && err.ok()) {
                const int b = (int) ((st - 1) % 3);
                // one stream for all chunks: kernels of consecutive chunks on
                // three streams, overlapping each other's ramp, measured 25 %
                // slower (57.5 vs 46.1 ms per 1 GiB; zero-copy kernels
                // running together get in each other's way).  The kernel
                // writes the page-locked buffer itself: a zero-copy kernel
                // that only reads host memory pays less at its end (~0.03 vs
                // ~0.12 ms, profiles/r03_zero_copy_split.json), but returning
                // the result from HBM with a copy engine while the next kernel
                // reads took 56 ms per GiB against 44.6
                // (profiles/r03_pageable_split_rejected.jsonl): the copy
                // engine and the CUs' PCIe reads share the link badly, as the
                // SDMA-only duplex pattern does (56 ms, bench.py pcie)
                int rc = enqueue(kernel_chunk(st - 1, b), P.ring.s, true);
                if (rc == MPIX_REDOP_SUCCESS)
                    rc = hip_err(hipEventRecord(P.ring.ev[b], P.ring.s));
                err.fail(rc);
                mark(st, w, 0);
            }
            if (st < n && err.ok()) {       // copy chunk st in
                char *h = P.ring.buf.host + (size_t) (st % 3) * 2 * half;
                size_t at, lo, len;
                part(st, w, &at, &lo, &len);
                if (len && in_pg)
                    copy_to_pinned(h + lo, (const char *) c.in + at + lo, len);
                if (len && io_pg)
                    copy_to_pinned(h + half + lo, (const char *) c.io + at + lo, len);
                mark(st, w, 1);
            }
            if (st >= 2 && st - 2 < n && err.ok()) {   // chunk st-2 out
                const int b = (int) ((st - 2) % 3);
                int rc = hip_err(hipEventSynchronize(P.ring.ev[b]));
                mark(st, w, 2);
                if (rc)
                    err.fail(rc);
                else if (io_pg) {
                    size_t at, lo, len;
                    part(st - 2, w, &at, &lo, &len);
                    if (len)
                        memcpy((char *) c.io + at + lo,
                               P.ring.buf.host + (size_t) b * 2 * half + half + lo, len);
                }
                mark(st, w, 3);
            }
            bar.wait();
            mark(st, w, 4);
        }
    };
    mpix::run_workers(W, cpus, work);
    (void) hipStreamSynchronize(P.ring.s);      // nothing left reading the buffers
    if (tr.on) {
        fprintf(stderr, "{\"wave_trace\": {\"W\": %d, \"ext\": %llu, \"chunks\": [", W,
                (unsigned long long) c.ext);
        for (int64_t k = 0; k < n; ++k)
            fprintf(stderr, "%s%llu", k ? "," : "", (unsigned long long) chunks[(size_t) k].count);
        fprintf(stderr, "], \"cpus\": [");
        for (int w = 0; w < W; ++w)
            fprintf(stderr, "%s%d", w ? "," : "", trace_cpu[(size_t) w]);
        fprintf(stderr, "], ");
        tr.print_ns(stderr);
    }
    return err.rc.load();
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev)
            (void) hipSetDevice(dev);
        else
            prev = -1;
    }
    ~DeviceGuard()
    {
        if (prev >= 0)
            (void) hipSetDevice(prev);
    }
};

// ------------------------------------------- split combiners' fixup words
// The words k_contig32 writes and k_fixup32 reads for a split combiner
// (redop_kernels.h is_split) live in buffers kept by redop_fixup.h's registry,
// which states the rules (one holder per key from acquire to release, a free
// only behind a completed event, at most kFixupMaxIdle idle buffers); these
// are its HIP operations.
struct FixupHipOps {
    void *alloc(int dev, size_t bytes)
    {
        DeviceGuard g(dev);
        void *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void) hipGetLastError();
            return nullptr;
        }
        return p;
    }
    void free(int dev, void *p)
    {
        DeviceGuard g(dev);
        (void) hipFree(p);
        (void) hipGetLastError();
    }
    void *record(int dev, uintptr_t stream, void *ev)
    {
        DeviceGuard g(dev);
        hipEvent_t e = (hipEvent_t) ev;
        // the event says only that the kernels before it are through with the
        // words (nobody reads results behind it): no timing, and no cache
        // write-back and invalidation between one call's kernels and the next's
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) !=
                      hipSuccess) {
            (void) hipGetLastError();
            return nullptr;
        }
        if (hipEventRecord(e, (hipStream_t) stream) != hipSuccess) {
            (void) hipGetLastError();
            if (!ev)
                (void) hipEventDestroy(e);
            return nullptr;
        }
        return e;
    }
    bool done(void *ev)
    {
        const hipError_t e = hipEventQuery((hipEvent_t) ev);
        if (e != hipSuccess)
            (void) hipGetLastError();
        return e == hipSuccess;
    }
    bool wait(void *ev)
    {
        const hipError_t e = hipEventSynchronize((hipEvent_t) ev);
        if (e != hipSuccess)
            (void) hipGetLastError();
        return e == hipSuccess;
    }
    void drop(int dev, void *ev)
    {
        DeviceGuard g(dev);
        (void) hipEventDestroy((hipEvent_t) ev);
    }
    bool sync(int dev, uintptr_t stream)
    {
        DeviceGuard g(dev);
        return hipStreamSynchronize((hipStream_t) stream) == hipSuccess;
    }
};
using FixupReg = mpix::FixupRegistry<FixupHipOps>;
FixupReg *g_fixup = new FixupReg(FixupHipOps{});    // never destroyed (no HIP call at exit)

// ------------------------------------------- peer access between devices
// A kernel on device `dev` may dereference another device's hipMalloc memory
// only once peer access dev -> owner is enabled.  The reference's HIP backend
// enables it for every device pair at init (yaksuri_hip_init_hooks.c:164-181:
// hipDeviceCanAccessPeer, then hipDeviceEnablePeerAccess, "already enabled"
// tolerated); here each pair is settled at its first use, once per process.
// State per ordered pair: 0 unknown, 1 direct access, 2 impossible (callers
// then copy with hipMemcpyPeerAsync or decline).  MPIX_REDOP_PEER=stage treats
// every pair as impossible (the staging path, testable on any 2-GPU box).
std::atomic<int8_t> g_peer[kMaxDev][kMaxDev];
std::mutex g_peer_mu;

enum PeerState : int8_t { kPeerUnknown = 0, kPeerDirect = 1, kPeerNone = 2, kPeerUnsure = 3 };

// kPeerDirect: kernels on `dev` may read `owner`'s memory; kPeerNone: the
// runtime says they may not (or MPIX_REDOP_PEER=stage); kPeerUnsure: the pair
// cannot even be asked (an owner index this process does not see, e.g. memory
// mapped from another process's GPU under a restricted HIP_VISIBLE_DEVICES) --
// used as it is, as the IPC mapping that produced it allows
PeerState peer_state(int dev, int owner)
{
    if (dev == owner)
        return kPeerDirect;
    int ndev = 0;
    if (dev < 0 || owner < 0 || dev >= kMaxDev || owner >= kMaxDev ||
        hipGetDeviceCount(&ndev) != hipSuccess || dev >= ndev || owner >= ndev) {
        (void) hipGetLastError();
        return kPeerUnsure;
    }
    int8_t st = g_peer[dev][owner].load(std::memory_order_acquire);
    if (st)
        return (PeerState) st;
    std::lock_guard<std::mutex> l(g_peer_mu);
    st = g_peer[dev][owner].load(std::memory_order_acquire);
    if (st)
        return (PeerState) st;
    const char *force = getenv("MPIX_REDOP_PEER");
    PeerState r;
    int can = 0;
    if (force && strcmp(force, "stage") == 0) {
        r = kPeerNone;
    } else if (hipDeviceCanAccessPeer(&can, dev, owner) != hipSuccess) {
        r = kPeerUnsure;
    } else if (!can) {
        r = kPeerNone;
    } else {
        DeviceGuard g(dev);
        hipError_t e = hipDeviceEnablePeerAccess(owner, 0);
        r = (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) ? kPeerDirect : kPeerNone;
    }
    (void) hipGetLastError();       // "already enabled" is sticky otherwise
    g_peer[dev][owner].store((int8_t) r, std::memory_order_release);
    return r;
}

bool peer_access(int dev, int owner) { return peer_state(dev, owner) == kPeerDirect; }

// The device a stream's kernels run on (the null stream: the current one).
int stream_device(hipStream_t s)
{
    int dev = 0;
    if (s) {
        hipDevice_t d;
        if (hipStreamGetDevice(s, &d) == hipSuccess)
            return (int) d;
        (void) hipGetLastError();
    }
    (void) hipGetDevice(&dev);
    return dev;
}

// The stream-ordered entry points take pointers a kernel on `s` can
// dereference: a pageable host pointer would fault the GPU and is refused with
// MPI_ERR_BUFFER; pinned host memory is translated to its device mapping; and
// another device's memory is reachable only with peer access (enabled here at
// first use), else refused too.  `launch` caches the stream's device (-2 = not
// looked up yet).
bool reachable(const void *p, hipStream_t s, int *launch, const void **devptr,
               bool *pinned = nullptr)
{
    int owner = -1;
    const Where w = classify(p, &owner, devptr);
    if (w == Where::Pageable)
        return false;
    if (w != Where::Device) {
        if (pinned)
            *pinned = true;     // page-locked host memory, read through its mapping
        return true;
    }
    if (*launch == -2)
        *launch = stream_device(s);
    return peer_state(*launch, owner) != kPeerNone;
}

// ------------------------------------------- derived targets as runs
// The runs, their scan, residue groups and tables and the committed plans'
// layout: redop_runs.h.  What follows uploads and launches.
using mpix::ResidueGroup;
using mpix::Run;
using mpix::RunTable;

// Upload a run table on `s` through the next of the current device's two
// slots, shared by the reduce and the fetch forms.  On success *slot holds the
// device copy (tab) and the caller records slot->done on `s` after the launches
// that read it; whenever *slot is set, also on an error, that record is owed.
int upload_runs(const RunTable &rt, hipStream_t s, DevState::IovSlot **slot)
{
    const size_t need = rt.tab.size();
    int dev = 0;
    (void) hipGetDevice(&dev);
    DevState *d = dev_state(dev);
    if (!d)
        return MPIX_REDOP_ERR_OTHER;
    DevState::IovSlot &sl = d->iov[d->iov_next++ & 1];
    if (!sl.done && hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) != hipSuccess)
        return MPIX_REDOP_ERR_OTHER;
    // the slot's previous table may still be read by kernels queued on any
    // stream (this thread may have used another one then): wait for them
    int rc = hip_err(hipEventSynchronize(sl.done));
    if (rc != MPIX_REDOP_SUCCESS)
        return rc;
    if (sl.cap < need) {
        if (sl.tab)
            (void) hipFree(sl.tab);
        if (sl.host)
            (void) hipHostFree(sl.host);
        sl.tab = nullptr;
        sl.host = nullptr;
        sl.cap = 0;
        if (hipMalloc((void **) &sl.tab, need * sizeof(int64_t)) != hipSuccess)
            return MPIX_REDOP_ERR_OTHER;
        if (hipHostMalloc((void **) &sl.host, need * sizeof(int64_t), hipHostMallocDefault) !=
            hipSuccess)
            return MPIX_REDOP_ERR_OTHER;
        sl.cap = need;
    }
    // the table goes through the pinned copy, so the upload is a true async
    // copy on s (no wait on the caller's stream); both copies are free for
    // reuse once sl.done, recorded after the launches, has fired
    *slot = &sl;
    memcpy(sl.host, rt.tab.data(), need * sizeof(int64_t));
    return hip_err(hipMemcpyAsync(sl.tab, sl.host, need * sizeof(int64_t), hipMemcpyHostToDevice,
                                  s));
}

// Group the runs, upload their table on `s`, launch every residue group
// through launch(group) (a hipError_t) and record the event the slot is owed.
template <class F>
int launch_groups(const std::vector<Run> &runs, int64_t e, hipStream_t s, F launch)
{
    RunTable rt;
    mpix::group_runs(runs, e, &rt);
    DevState::IovSlot *sl = nullptr;
    int rc = upload_runs(rt, s, &sl);
    for (size_t g = 0; g < rt.resid.size() && rc == MPIX_REDOP_SUCCESS; ++g)
        rc = hip_err(launch(ResidueGroup(rt, g, sl->tab)));
    if (!sl)
        return rc;
    const int rc2 = hip_err(hipEventRecord(sl->done, s));
    return rc ? rc : rc2;
}

// Enqueue a list of runs on `s`.  Runs are split by their offset modulo the
// extent so each launch indexes inout in whole elements from one base
// (inout + residue); the source offset table keeps the packed source in the
// original run order.
int enqueue_runs(const void *inbuf, void *inoutbuf, const std::vector<Run> &runs, uint32_t dt,
                 uint32_t op, hipStream_t s)
{
    uint32_t it;
    uint64_t ext;
    int rc = validate(inbuf, inoutbuf, 0, dt, op, &it, &ext);
    if (rc != MPIX_REDOP_SUCCESS)
        return rc;
    int64_t total = 0;
    for (const Run &r : runs)
        total += r.n;
    if (total == 0)
        return MPIX_REDOP_SUCCESS;
    if (no_buffer(inbuf) || no_buffer(inoutbuf))
        return MPIX_REDOP_ERR_BUFFER;
    {
        const void *pin, *pio;
        int launch = -2;
        if (!reachable(inbuf, s, &launch, &pin) || !reachable(inoutbuf, s, &launch, &pio))
            return MPIX_REDOP_ERR_BUFFER;
        inbuf = pin;
        inoutbuf = (void *) pio;
    }
    const int64_t e = (int64_t) ext;
    if (!mpix::residues_aligned(runs, e))
        return MPIX_REDOP_ERR_ARG;
    uint32_t opi = op & 0xf;
    if (opi == kOpNoOp)
        return MPIX_REDOP_SUCCESS;
    if (opi == kOpReplace) {    // one typemap copy per run
        int64_t src = 0;
        for (size_t k = 0; k < runs.size() && rc == MPIX_REDOP_SUCCESS; ++k) {
            rc = replace_rows((char *) inoutbuf + runs[k].off, ext,
                              (const char *) inbuf + src * e, ext, (uint64_t) runs[k].n, it, ext, s);
            src += runs[k].n;
        }
        return rc;
    }
    const Entry *en = gpu_entry(opi, it);
    if (!en)
        return MPIX_REDOP_ERR_TYPE;
    return launch_groups(runs, e, s, [&](const ResidueGroup &g) {
        return en->iov(inbuf, (char *) inoutbuf + g.resid, g.seg_off, g.prefix, g.src_off, g.n,
                       g.total, params(), launch_cfg(), s);
    });
}

// ------------------------------------------- the RMA-style entries' scaffolding
// One operand rule, one placement and one synchronous tail for the fused
// get-accumulate, its iov and plan forms and the element-atomic entries
// (mpix_redop.h numbers the checks; every family calls these in that order).
// fetch: the call has a result.  reads_origin: the origin is an operand (not
// under the fetch forms' MPI_NO_OP, where it may be NULL).

// The no-buffer check: an operand that is NULL or MPI_IN_PLACE.
bool missing_operand(const void *origin, const void *result, const void *target, bool fetch,
                     bool reads_origin)
{
    return (fetch && no_buffer(result)) || no_buffer(target) || (reads_origin && no_buffer(origin));
}

// The overlap check: the byte ranges of result and origin against the target's
// bounding range (`span` bytes from target_lo) and against each other.
bool operands_overlap(const void *origin, uint64_t origin_bytes, const void *result,
                      uint64_t result_bytes, const void *target_lo, uint64_t span, bool fetch,
                      bool reads_origin)
{
    return (fetch && ranges_overlap(result, result_bytes, target_lo, span)) ||
           (reads_origin && (ranges_overlap(origin, origin_bytes, target_lo, span) ||
                             (fetch && ranges_overlap(origin, origin_bytes, result, result_bytes))));
}

// ... with result and origin packed (`packed` bytes each)
bool operands_overlap(const void *origin, const void *result, const void *target_lo,
                      uint64_t packed, uint64_t span, bool fetch, bool reads_origin)
{
    return operands_overlap(origin, packed, result, packed, target_lo, span, fetch, reads_origin);
}

// The operands as a kernel on the stream dereferences them (reachable): filled
// with the caller's pointers, translated in place -- result, target, origin,
// in that order.  own_target: the caller has placed the target by a rule of
// its own (atomic_target_ok) and set `launch`.
struct Placed {
    const void *origin, *result, *target;
    int launch = -2;        // the stream's device, once a device operand asked for it
    bool zc = false;        // an operand is page-locked host memory
};

bool place_operands(Placed *p, bool fetch, bool own_target, bool reads_origin, hipStream_t s)
{
    return (!fetch || reachable(p->result, s, &p->launch, &p->result, &p->zc)) &&
           (own_target || reachable(p->target, s, &p->launch, &p->target, &p->zc)) &&
           (!reads_origin || reachable(p->origin, s, &p->launch, &p->origin, &p->zc));
}

// The synchronous forms: a device-memory target, the calling thread's library
// stream of that device, and a wait on it (no in-kernel completion word).
template <class F>
int on_library_stream(const void *target, F enqueue)
{
    int dev = 0;
    const void *dp;
    if (classify(target, &dev, &dp) != Where::Device)
        return MPIX_REDOP_ERR_BUFFER;
    DeviceGuard guard(dev);
    DevState *d = dev_state(dev);
    if (!d)
        return MPIX_REDOP_ERR_OTHER;
    const int rc = enqueue(d->s[0]);
    const int rc2 = wait_stream(d, d->s[0]);
    return rc ? rc : rc2;
}

// Validated arguments of either form of an entry: enqueue on the caller's
// stream, or (sync) through on_library_stream.
template <class F>
int on_stream(bool sync, hipStream_t s, const void *target, F enqueue)
{
    return sync ? on_library_stream(target, enqueue) : enqueue(s);
}

// What the copy kernels of MPI_NO_OP / MPI_REPLACE do (redop_dispatch.h).
mpix::CopyMode copy_mode(uint32_t opi, bool fetch)
{
    return !fetch ? mpix::kCopyStore : opi == kOpReplace ? mpix::kCopySwap : mpix::kCopyFetch;
}

}  // namespace

namespace mpix {
FixupLease fixup_acquire(hipStream_t s, size_t bytes)
{
    int dev = 0;
    if (hipStreamGetDevice(s, &dev) != hipSuccess) {
        (void) hipGetLastError();
        return FixupLease{};
    }
    // hipStreamPerThread is one handle value and a stream of its own in every thread
    const FixupKey key{dev, (uintptr_t) s, s == hipStreamPerThread ? fixup_thread_token() : 0};
    const FixupReg::Lease l = g_fixup->acquire(key, bytes);
    return FixupLease{static_cast<uint64_t *>(l.ptr), l.entry};
}

void fixup_release(const FixupLease &lease)
{
    g_fixup->release(FixupReg::Lease{lease.words, lease.entry});
}
}  // namespace mpix

extern "C" {

int MPIX_Redop_init(void)
{
    launch_cfg();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return set_err(MPIX_REDOP_ERR_OTHER);
    return set_err(dev_state(dev) ? MPIX_REDOP_SUCCESS : MPIX_REDOP_ERR_OTHER);
}

static void free_states(DevState *arr)
{
    for (int i = 0; i < kMaxDev; ++i) {
        DevState &d = arr[i];
        if (!d.init)
            continue;
        DeviceGuard g(i);
        for (int k = 0; k < 2; ++k)
            if (d.s[k])
                (void) hipStreamDestroy(d.s[k]);
        if (d.done)
            (void) hipEventDestroy(d.done);
        if (d.flag)
            (void) hipHostFree((void *) d.flag);
        if (d.flag_ctr)
            (void) hipFree(d.flag_ctr);
        if (d.scratch)
            (void) hipFree(d.scratch);
        for (DevState::IovSlot &sl : d.iov) {
            if (sl.done) {
                (void) hipEventSynchronize(sl.done);
                (void) hipEventDestroy(sl.done);
            }
            if (sl.tab)
                (void) hipFree(sl.tab);
            if (sl.host)
                (void) hipHostFree(sl.host);
        }
        d.bounce.free();
        for (hipEvent_t e : d.tev)
            (void) hipEventDestroy(e);
        d = DevState();
    }
    delete[] arr;
}

int MPIX_Redop_finalize(void)
{
    g_fixup->finalize();
    std::vector<DevState *> pooled;
    {
        std::lock_guard<std::mutex> l(g_pool_mu);
        pooled.swap(*g_pool);
    }
    if (t_dev.arr)
        pooled.push_back(t_dev.arr);
    t_dev.arr = nullptr;
    for (DevState *arr : pooled)
        free_states(arr);
    for (int i = 0; i < kMaxDev; ++i) {     // the process-wide pageable worker slots
        PipeSet &P = g_pipes[i];
        std::lock_guard<std::mutex> l(P.mu);
        if (!P.slot[0].s && !P.slot[0].buf.host && !P.ring.buf.host && !P.ring.s)
            continue;
        DeviceGuard g(i);
        // a slot's stream (synchronised first), its events and its pinned buffer
        auto release = [](PipeSlot &sl) {
            if (sl.s) {
                (void) hipStreamSynchronize(sl.s);
                (void) hipStreamDestroy(sl.s);
            }
            for (hipEvent_t e : sl.ev)
                if (e)
                    (void) hipEventDestroy(e);
            sl.buf.free();
            sl = PipeSlot();
        };
        for (PipeSlot &sl : P.slot)
            release(sl);
        P.half = 0;
        P.nbuf = 0;
        release(P.ring);
    }
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Reduce_local_async(const void *inbuf, void *inoutbuf, MPIX_Aint count,
                            MPIX_Datatype datatype, MPIX_Op op, void *stream)
{
    uint32_t it;
    uint64_t ext;
    int rc = validate(inbuf, inoutbuf, count, (uint32_t) datatype, (uint32_t) op, &it, &ext);
    if (rc != MPIX_REDOP_SUCCESS || count == 0)
        return set_err(rc);
    const void *pin, *pio;
    int launch = -2;
    bool zc = false;
    if (!reachable(inbuf, (hipStream_t) stream, &launch, &pin, &zc) ||
        !reachable(inoutbuf, (hipStream_t) stream, &launch, &pio, &zc))
        return set_err(MPIX_REDOP_ERR_BUFFER);
    return set_err(enqueue(Combine{pin, (void *) pio, (uint64_t) count, it, ext, (uint32_t) op},
                           (hipStream_t) stream, zc));
}

// Several ready chunks in one launch (include/mpix_redop.h).  Checks first,
// all before any device work: the arguments, then that no triple's target
// overlaps another triple's target or source (the batch runs them in no
// particular order), then that the stream's device can reach every operand.
static_assert(mpix::kMaxBatchSegs == MPIX_BATCH_MAX, "one batch limit");

int MPIX_Reduce_local_batch_async(const void *const *inbufs, void *const *inoutbufs,
                                  const MPIX_Aint *counts, int k, MPIX_Datatype datatype,
                                  MPIX_Op op, void *stream)
{
    if (k < 1 || k > MPIX_BATCH_MAX || !inbufs || !inoutbufs || !counts)
        return set_err(MPIX_REDOP_ERR_ARG);
    uint32_t it = 0;
    uint64_t ext = 0;
    for (int i = 0; i < k; ++i) {
        int rc = validate(inbufs[i], inoutbufs[i], counts[i], (uint32_t) datatype, (uint32_t) op,
                          &it, &ext);
        if (rc != MPIX_REDOP_SUCCESS)
            return set_err(rc);
    }
    for (int i = 0; i < k; ++i) {
        if (!counts[i])
            continue;
        const uint64_t bi = (uint64_t) counts[i] * ext;
        for (int j = 0; j < k; ++j) {
            if (j == i || !counts[j])
                continue;
            const uint64_t bj = (uint64_t) counts[j] * ext;
            const uintptr_t ti = (uintptr_t) inoutbufs[i], tj = (uintptr_t) inoutbufs[j],
                            sj = (uintptr_t) inbufs[j];
            if ((ti < tj + bj && tj < ti + bi) || (ti < sj + bj && sj < ti + bi))
                return set_err(MPIX_REDOP_ERR_BUFFER);
        }
    }
    const uint32_t opi = (uint32_t) op & 0xf;
    const Entry *e = (opi >= kOpReplace) ? nullptr : gpu_entry(opi, it);
    if (opi < kOpReplace && !e)
        return set_err(MPIX_REDOP_ERR_TYPE);
    const void *pin[MPIX_BATCH_MAX];
    void *pio[MPIX_BATCH_MAX];
    uint64_t cnt[MPIX_BATCH_MAX];
    bool zc[MPIX_BATCH_MAX];
    int m = 0, launch = -2;
    for (int i = 0; i < k; ++i) {
        if (!counts[i])
            continue;
        const void *a, *b;
        bool pinned = false;
        if (!reachable(inbufs[i], (hipStream_t) stream, &launch, &a, &pinned) ||
            !reachable(inoutbufs[i], (hipStream_t) stream, &launch, &b, &pinned))
            return set_err(MPIX_REDOP_ERR_BUFFER);
        pin[m] = a;
        pio[m] = (void *) b;
        zc[m] = pinned;
        cnt[m++] = (uint64_t) counts[i];
    }
    if (!m)
        return set_err(MPIX_REDOP_SUCCESS);
    // REPLACE / NO_OP / EQUAL, and every triple with a page-locked host
    // operand: a call each -- a kernel reading host memory over PCIe runs the
    // capped, looping zero-copy grid (g_zc_grid), which the
    // batch kernels' one-tile-per-block layout cannot.  The triples are
    // independent (checked above), so their order does not matter.
    int nd = 0;
    for (int i = 0; i < m; ++i) {
        if (!e || zc[i]) {
            int rc = enqueue(Combine{pin[i], pio[i], cnt[i], it, ext, (uint32_t) op},
                             (hipStream_t) stream, zc[i]);
            if (rc != MPIX_REDOP_SUCCESS)
                return set_err(rc);
            continue;
        }
        pin[nd] = pin[i];
        pio[nd] = pio[i];
        cnt[nd++] = cnt[i];
    }
    if (!nd)
        return set_err(MPIX_REDOP_SUCCESS);
    return set_err(hip_err(e->batch(pin, pio, cnt, nd, params(), launch_cfg(), (hipStream_t) stream)));
}

int MPIX_Reduce_local(const void *inbuf, void *inoutbuf, MPIX_Aint count, MPIX_Datatype datatype,
                      MPIX_Op op)
{
    uint32_t it;
    uint64_t ext;
    int rc = validate(inbuf, inoutbuf, count, (uint32_t) datatype, (uint32_t) op, &it, &ext);
    if (rc != MPIX_REDOP_SUCCESS || count == 0)
        return set_err(rc);
    uint32_t opi = (uint32_t) op & 0xf;
    if (opi == kOpEqual ? ((it & 0xffffff00u) != U8 || count < 8)
                        : (opi != kOpReplace && opi != kOpNoOp && !gpu_entry(opi, it)))
        return set_err(MPIX_REDOP_ERR_TYPE);
    launch_cfg();
    int din = -1, dio = -1, cur = 0;
    (void) hipGetDevice(&cur);
    const void *pin, *pio;
    Where win = classify(inbuf, &din, &pin);
    Where wio = classify(inoutbuf, &dio, &pio);
    int dev = wio == Where::Device ? dio : (win == Where::Device ? din : cur);
    DeviceGuard guard(dev);
    const mpix::HostCall call{win, wio,
                              win == Where::Device && wio == Where::Device && din != dio &&
                                  peer_state(dio, din) == kPeerNone,
                              (uint64_t) count * ext, opi == kOpEqual,
                              g_zero_copy.load(), g_bounce_bytes, g_pipe_threads.load(),
                              g_pipe_wave.load() != 0, g_pipe_chunk.load()};
    const int peer = call.no_peer ? din : -1;   // `in`'s device, copied from with PeerAsync
    // a form that cannot have its buffers answers -1: the next one, then
    for (mpix::Route declined = mpix::Route::None;;) {
        const mpix::HostRoute r = mpix::host_route(call, declined);
        // an operand the form copies itself as the caller gave it, another
        // as the device sees it
        const Combine c{r.in_host ? inbuf : pin, r.io_host ? inoutbuf : (void *) pio,
                        (uint64_t) count, it, ext, (uint32_t) op};
        // the wave and worker forms have streams of their own, the others
        // use the calling thread's
        const bool pipes = r.route == mpix::Route::Wave || r.route == mpix::Route::Worker;
        DevState *d = pipes ? nullptr : dev_state(dev);
        if (!pipes && !d)
            return set_err(MPIX_REDOP_ERR_OTHER);
        switch (r.route) {
            case mpix::Route::PeerStaged:
            case mpix::Route::Staged: rc = staged(d, c, r.in_host, r.io_host, dev, peer); break;
            case mpix::Route::PeerEqual:
            case mpix::Route::EqualWhole:
                rc = equal_whole(d, c, r.in_host, r.io_host, dev, peer);
                break;
            case mpix::Route::Bounce: rc = bounced(d, c, r.in_host, r.io_host); break;
            case mpix::Route::Wave: rc = waved(c, r.in_host, r.io_host, dev, call.threads); break;
            case mpix::Route::Worker:
                rc = pipelined(c, r.in_host, r.io_host, dev, call.threads);
                break;
            default: rc = run_sync(d, c, r.zero_copy);
        }
        if (rc >= 0)
            return set_err(rc);
        declined = r.route;
    }
}

int MPIX_Reduce_local_vector_async(const void *inbuf, void *inoutbuf, MPIX_Aint count,
                                   MPIX_Aint blocklen, MPIX_Aint stride,
                                   MPIX_Datatype basic_type, MPIX_Op op, void *stream)
{
    if (count < 0 || blocklen < 0)
        return set_err(MPIX_REDOP_ERR_COUNT);
    if (stride < blocklen)
        return set_err(MPIX_REDOP_ERR_ARG);     // overlapping target runs
    uint32_t it;
    uint64_t ext;
    int rc = validate(inbuf, inoutbuf, 0, (uint32_t) basic_type, (uint32_t) op, &it, &ext);
    if (rc != MPIX_REDOP_SUCCESS)
        return set_err(rc);
    uint64_t n = (uint64_t) count * (uint64_t) blocklen;
    if (n == 0)
        return set_err(MPIX_REDOP_SUCCESS);
    if (no_buffer(inbuf) || no_buffer(inoutbuf))
        return set_err(MPIX_REDOP_ERR_BUFFER);
    uint64_t span = ((uint64_t) (count - 1) * (uint64_t) stride + (uint64_t) blocklen) * ext;
    if (ranges_overlap(inbuf, n * ext, inoutbuf, span))
        return set_err(MPIX_REDOP_ERR_BUFFER);
    {
        const void *pin, *pio;
        int launch = -2;
        if (!reachable(inbuf, (hipStream_t) stream, &launch, &pin) ||
            !reachable(inoutbuf, (hipStream_t) stream, &launch, &pio))
            return set_err(MPIX_REDOP_ERR_BUFFER);
        inbuf = pin;
        inoutbuf = (void *) pio;
    }
    uint32_t opi = (uint32_t) op & 0xf;
    if (opi == kOpNoOp)
        return set_err(MPIX_REDOP_SUCCESS);
    if (opi == kOpReplace)
        return set_err(copy_blocks(inoutbuf, (uint64_t) stride, inbuf, (uint64_t) blocklen,
                                   (uint64_t) count, (uint64_t) blocklen, it, ext,
                                   (hipStream_t) stream));
    const Entry *e = gpu_entry(opi, it);
    if (!e)
        return set_err(MPIX_REDOP_ERR_TYPE);
    return set_err(hip_err(e->vector(inbuf, inoutbuf, (uint64_t) count, (uint64_t) blocklen,
                                     (uint64_t) stride, params(), launch_cfg(),
                                     (hipStream_t) stream)));
}

// the target is classified before anything is validated: the whole
// stream-ordered call runs on the library stream
int MPIX_Reduce_local_vector(const void *inbuf, void *inoutbuf, MPIX_Aint count,
                             MPIX_Aint blocklen, MPIX_Aint stride, MPIX_Datatype basic_type,
                             MPIX_Op op)
{
    return set_err(on_library_stream(inoutbuf, [&](hipStream_t s) {
        return MPIX_Reduce_local_vector_async(inbuf, inoutbuf, count, blocklen, stride,
                                              basic_type, op, s);
    }));
}

// ------------------------------------------------ fused get-accumulate
// One implementation for both forms: the contiguous one is the vector target
// with blocklen = stride = 1.
// Every check that needs no device: on success *n holds the packed element
// count (0: nothing to do, no pointer was looked at).
static int getacc_validate(const void *origin, const void *result, const void *target,
                           MPIX_Aint count, MPIX_Aint blocklen, MPIX_Aint stride, uint32_t dt,
                           uint32_t op, uint32_t *it, uint64_t *ext, uint64_t *n)
{
    *n = 0;
    if (count < 0 || blocklen < 0)
        return MPIX_REDOP_ERR_COUNT;
    if (stride < blocklen)
        return MPIX_REDOP_ERR_ARG;      // overlapping target runs
    if (is_builtin_op(op) && (op & 0xf) == kOpEqual)
        return MPIX_REDOP_ERR_OP;       // MPIX_EQUAL is no accumulate op
    int rc = validate(nullptr, nullptr, 0, dt, op, it, ext);
    if (rc != MPIX_REDOP_SUCCESS || count == 0 || blocklen == 0)
        return rc;
    // no operand spans 2^56 bytes (validate's cap), the target's span included
    const uint64_t cap = ((uint64_t) 1 << 56) / *ext;
    const uint64_t c = (uint64_t) count, bl = (uint64_t) blocklen, st = (uint64_t) stride;
    if (bl > cap || c > cap / bl || (c > 1 && st > (cap - bl) / (c - 1)))
        return MPIX_REDOP_ERR_COUNT;
    const uint32_t opi = op & 0xf;
    const bool reads_origin = opi != kOpNoOp;
    if (missing_operand(origin, result, target, true, reads_origin))
        return MPIX_REDOP_ERR_BUFFER;
    if (operands_overlap(origin, result, target, c * bl * *ext, ((c - 1) * st + bl) * *ext, true,
                         reads_origin))
        return MPIX_REDOP_ERR_BUFFER;
    if (opi < kOpReplace && !getacc_entry(opi, *it))
        return MPIX_REDOP_ERR_TYPE;     // a legal pair without a kernel
    *n = c * bl;
    return MPIX_REDOP_SUCCESS;
}

// Placed operands: the launch on `s`.  NO_OP and REPLACE are the stream-ordered
// copies (fetch, then replace); every other op is one fused kernel.
static int getacc_launch(const void *po, void *pr, void *pt, uint64_t count, uint64_t bl,
                         uint64_t st, uint32_t it, uint64_t ext, uint32_t opi, bool zc,
                         hipStream_t s)
{
    if (opi == kOpReplace || opi == kOpNoOp) {
        int rc = copy_blocks(pr, bl, pt, st, count, bl, it, ext, s);
        if (rc == MPIX_REDOP_SUCCESS && opi == kOpReplace)
            rc = copy_blocks(pt, st, po, bl, count, bl, it, ext, s);
        return rc;
    }
    const mpix::GetaccEntry *e = getacc_entry(opi, it);
    if (!e)
        return MPIX_REDOP_ERR_TYPE;
    if (bl == st)
        return hip_err(e->contig(po, pr, pt, count * bl, params(), launch_cfg(zc), s));
    return hip_err(e->vector(po, pr, pt, count, bl, st, params(), launch_cfg(), s));
}

// Either form (sync: on the library stream): validate once, then placement
// and the launch.
static int getacc(const void *origin, void *result, void *target, MPIX_Aint count,
                  MPIX_Aint blocklen, MPIX_Aint stride, uint32_t dt, uint32_t op, bool sync,
                  hipStream_t stream)
{
    uint32_t it;
    uint64_t ext, n;
    int rc = getacc_validate(origin, result, target, count, blocklen, stride, dt, op, &it, &ext, &n);
    if (rc != MPIX_REDOP_SUCCESS || n == 0)
        return rc;
    return on_stream(sync, stream, target, [&](hipStream_t s) {
        const uint32_t opi = op & 0xf;
        Placed p{origin, result, target};
        if (!place_operands(&p, true, false, opi != kOpNoOp, s))
            return MPIX_REDOP_ERR_BUFFER;
        return getacc_launch(p.origin, (void *) p.result, (void *) p.target, (uint64_t) count,
                             (uint64_t) blocklen, (uint64_t) stride, it, ext, opi, p.zc, s);
    });
}

int MPIX_Get_accumulate_local_async(const void *origin, void *result, void *target,
                                    MPIX_Aint count, MPIX_Datatype datatype, MPIX_Op op,
                                    void *stream)
{
    return set_err(getacc(origin, result, target, count, 1, 1, (uint32_t) datatype, (uint32_t) op,
                          false, (hipStream_t) stream));
}

int MPIX_Get_accumulate_local(const void *origin, void *result, void *target, MPIX_Aint count,
                              MPIX_Datatype datatype, MPIX_Op op)
{
    return set_err(getacc(origin, result, target, count, 1, 1, (uint32_t) datatype, (uint32_t) op,
                          true, nullptr));
}

int MPIX_Get_accumulate_local_vector_async(const void *origin, void *result, void *target,
                                           MPIX_Aint count, MPIX_Aint blocklen, MPIX_Aint stride,
                                           MPIX_Datatype basic_type, MPIX_Op op, void *stream)
{
    return set_err(getacc(origin, result, target, count, blocklen, stride, (uint32_t) basic_type,
                          (uint32_t) op, false, (hipStream_t) stream));
}

int MPIX_Get_accumulate_local_vector(const void *origin, void *result, void *target,
                                     MPIX_Aint count, MPIX_Aint blocklen, MPIX_Aint stride,
                                     MPIX_Datatype basic_type, MPIX_Op op)
{
    return set_err(getacc(origin, result, target, count, blocklen, stride, (uint32_t) basic_type,
                          (uint32_t) op, true, nullptr));
}

// The element runs of a caller's table (redop_runs.h); the iovec form's handle
// is resolved here, an unknown type going in as extent 0.
using mpix::runs_from_iov;

static int runs_from_iovec(MPIX_Aint nseg, const MPIX_Aint *iov_offsets, const MPIX_Aint *iov_lens,
                           uint32_t basic_type, std::vector<Run> *runs)
{
    const uint32_t it = to_internal(basic_type);
    return mpix::runs_from_iovec(nseg, iov_offsets, iov_lens, it == kNull ? 0 : size_of(it),
                                 it == kNull ? 0 : extent_of(it), runs);
}

int MPIX_Reduce_local_iov_async(const void *inbuf, void *inoutbuf, MPIX_Aint nseg,
                                const MPIX_Aint *seg_offsets, const MPIX_Aint *seg_counts,
                                MPIX_Datatype basic_type, MPIX_Op op, void *stream)
{
    std::vector<Run> runs;
    int rc = runs_from_iov(nseg, seg_offsets, seg_counts, &runs);
    if (rc != MPIX_REDOP_SUCCESS)
        return set_err(rc);
    return set_err(enqueue_runs(inbuf, inoutbuf, runs, (uint32_t) basic_type, (uint32_t) op,
                                (hipStream_t) stream));
}

int MPIX_Reduce_local_iovec_async(const void *inbuf, void *inoutbuf, MPIX_Aint nseg,
                                  const MPIX_Aint *iov_offsets, const MPIX_Aint *iov_lens,
                                  MPIX_Datatype basic_type, MPIX_Op op, void *stream)
{
    std::vector<Run> runs;
    int rc = runs_from_iovec(nseg, iov_offsets, iov_lens, (uint32_t) basic_type, &runs);
    if (rc != MPIX_REDOP_SUCCESS)
        return set_err(rc);
    return set_err(enqueue_runs(inbuf, inoutbuf, runs, (uint32_t) basic_type, (uint32_t) op,
                                (hipStream_t) stream));
}

// The fetch form over runs.  Every check that needs no device comes first, in
// the reduce form's order where it has the check too; then operand placement,
// and only then the table upload and the launches: one per residue group, the
// copy kernel for MPI_NO_OP / MPI_REPLACE, the combiner's fused kernel else.
static int getacc_runs(const void *origin, void *result, void *target,
                       const std::vector<Run> &runs, uint32_t dt, uint32_t op, hipStream_t s)
{
    uint32_t it;
    uint64_t ext;
    int rc = validate(nullptr, nullptr, 0, dt, op, &it, &ext);
    if (rc != MPIX_REDOP_SUCCESS)
        return rc;
    const uint32_t opi = op & 0xf;
    if (opi == kOpEqual)
        return MPIX_REDOP_ERR_OP;       // MPIX_EQUAL is no accumulate op
    const mpix::RunScan sc = mpix::scan_runs(runs, ext);
    if (!sc.over && sc.total == 0)
        return MPIX_REDOP_SUCCESS;
    const bool reads_origin = opi != kOpNoOp;
    if (missing_operand(origin, result, target, true, reads_origin))
        return MPIX_REDOP_ERR_BUFFER;
    const int64_t e = (int64_t) ext;
    if (!mpix::residues_aligned(runs, e))
        return MPIX_REDOP_ERR_ARG;
    if (sc.too_long(ext))
        return MPIX_REDOP_ERR_COUNT;
    if (operands_overlap(origin, result, (const char *) target + (int64_t) sc.lo, sc.total * ext,
                         (uint64_t) (sc.hi - sc.lo), true, reads_origin))
        return MPIX_REDOP_ERR_BUFFER;
    const mpix::GetaccIovEntry *en = nullptr;
    if (opi < kOpReplace && !(en = getacc_iov_entry(opi, it)))
        return MPIX_REDOP_ERR_TYPE;     // a legal pair without a kernel
    Placed p{origin, result, target};
    if (!place_operands(&p, true, false, reads_origin, s))
        return MPIX_REDOP_ERR_BUFFER;
    PairMap pm{0, 0};
    (void) padded_pair(it, &pm);
    return launch_groups(runs, e, s, [&](const ResidueGroup &g) {
        void *tg = (char *) p.target + g.resid;
        if (en)
            return en->iov(p.origin, (void *) p.result, tg, g.seg_off, g.prefix, g.src_off, g.n,
                           g.total, params(), launch_cfg(), s);
        return mpix::launch_getacc_iov_copy(copy_mode(opi, true), (uint32_t) ext, pm.value_bytes,
                                            pm.loc_off, p.origin, (void *) p.result, tg, g.seg_off,
                                            g.prefix, g.src_off, g.n, g.total, launch_cfg(), s);
    });
}

int MPIX_Get_accumulate_local_iov_async(const void *origin, void *result, void *target,
                                        MPIX_Aint nseg, const MPIX_Aint *seg_offsets,
                                        const MPIX_Aint *seg_counts, MPIX_Datatype basic_type,
                                        MPIX_Op op, void *stream)
{
    std::vector<Run> runs;
    int rc = runs_from_iov(nseg, seg_offsets, seg_counts, &runs);
    if (rc != MPIX_REDOP_SUCCESS)
        return set_err(rc);
    return set_err(getacc_runs(origin, result, target, runs, (uint32_t) basic_type, (uint32_t) op,
                               (hipStream_t) stream));
}

int MPIX_Get_accumulate_local_iovec_async(const void *origin, void *result, void *target,
                                          MPIX_Aint nseg, const MPIX_Aint *iov_offsets,
                                          const MPIX_Aint *iov_lens, MPIX_Datatype basic_type,
                                          MPIX_Op op, void *stream)
{
    std::vector<Run> runs;
    int rc = runs_from_iovec(nseg, iov_offsets, iov_lens, (uint32_t) basic_type, &runs);
    if (rc != MPIX_REDOP_SUCCESS)
        return set_err(rc);
    return set_err(getacc_runs(origin, result, target, runs, (uint32_t) basic_type, (uint32_t) op,
                               (hipStream_t) stream));
}

// ------------------------------------------------ committed iov plans
// What MPI_Type_commit is to a datatype: the layout of one (table, basic type)
// (mpix::PlanLayout, redop_runs.h), kept on the host and, after
// MPIX_Iov_plan_prepare, resident on each device that uses it.  The
// plan-taking entries then do no table work, no upload and no event call.
// Immutable after create apart from `dev` (behind `mu`; a launch reads its
// device's pointer with one acquire load).
struct MPIX_Iov_plan_s : mpix::PlanLayout {
    std::mutex mu;
    std::atomic<char *> dev[kMaxDev] = {};
    std::atomic<char *> pk_dev[kMaxDev] = {};
    explicit MPIX_Iov_plan_s(mpix::PlanLayout &&lay) : mpix::PlanLayout(std::move(lay)) {}
};

// Either table form.  *plan = NULL before anything else, nseg > INT_MAX before
// the table is read (typerep_op.c:111 asserts the same), and the plan pointer
// is looked at only after the table's own checks.
static int plan_create(MPIX_Aint nseg, const MPIX_Aint *offsets, const MPIX_Aint *second,
                       uint32_t basic_type, bool iovec, MPIX_Iov_plan *plan)
{
    if (plan)
        *plan = nullptr;
    if (nseg > (MPIX_Aint) INT_MAX)
        return MPIX_REDOP_ERR_COUNT;
    std::vector<Run> runs;
    int rc = iovec ? runs_from_iovec(nseg, offsets, second, basic_type, &runs)
                   : runs_from_iov(nseg, offsets, second, &runs);
    if (rc != MPIX_REDOP_SUCCESS)
        return rc;
    const uint32_t it = to_internal(basic_type);
    const uint64_t ext = it == kNull ? 0 : extent_of(it);
    if (ext == 0)
        return MPIX_REDOP_ERR_TYPE;
    mpix::PlanLayout lay;
    rc = lay.build(runs, it, ext);
    if (rc == MPIX_REDOP_SUCCESS && !plan)
        rc = MPIX_REDOP_ERR_ARG;
    if (rc == MPIX_REDOP_SUCCESS)
        *plan = new MPIX_Iov_plan_s(std::move(lay));
    return rc;
}

int MPIX_Iov_plan_create(MPIX_Aint nseg, const MPIX_Aint *seg_offsets, const MPIX_Aint *seg_counts,
                         MPIX_Datatype basic_type, MPIX_Iov_plan *plan)
{
    return set_err(plan_create(nseg, seg_offsets, seg_counts, (uint32_t) basic_type, false, plan));
}

int MPIX_Iov_plan_create_iovec(MPIX_Aint nseg, const MPIX_Aint *iov_offsets,
                               const MPIX_Aint *iov_lens, MPIX_Datatype basic_type,
                               MPIX_Iov_plan *plan)
{
    return set_err(plan_create(nseg, iov_offsets, iov_lens, (uint32_t) basic_type, true, plan));
}

// One of the plan's two table sets on `dev` (`slot`: dev[] or pk_dev[]; `bytes`
// in all, the first `na` from `a`, the rest from `b`), uploaded if it is not
// there yet (blocking), published with a release store behind the plan's mutex.
static int plan_upload(MPIX_Iov_plan_s *p, std::atomic<char *> *slot, int dev, size_t bytes,
                       const void *a, size_t na, const void *b, char **tab)
{
    *tab = nullptr;
    if (dev < 0 || dev >= kMaxDev)
        return MPIX_REDOP_ERR_OTHER;
    if (bytes == 0)
        return MPIX_REDOP_SUCCESS;
    if ((*tab = slot[dev].load(std::memory_order_acquire)))
        return MPIX_REDOP_SUCCESS;
    std::lock_guard<std::mutex> l(p->mu);
    if ((*tab = slot[dev].load(std::memory_order_acquire)))
        return MPIX_REDOP_SUCCESS;
    DeviceGuard guard(dev);
    char *d = nullptr;
    int rc = hip_err(hipMalloc((void **) &d, bytes));
    if (rc != MPIX_REDOP_SUCCESS) {
        (void) hipGetLastError();
        return rc;
    }
    rc = hip_err(hipMemcpy(d, a, na, hipMemcpyHostToDevice));
    if (rc == MPIX_REDOP_SUCCESS && bytes > na)
        rc = hip_err(hipMemcpy(d + na, b, bytes - na, hipMemcpyHostToDevice));
    if (rc != MPIX_REDOP_SUCCESS) {
        (void) hipFree(d);
        return rc;
    }
    slot[dev].store(d, std::memory_order_release);
    *tab = d;
    return MPIX_REDOP_SUCCESS;
}

// The plan's residue-group tables on `dev`: rt.tab, then tile.
static int plan_tables(MPIX_Iov_plan_s *p, int dev, char **tab)
{
    return plan_upload(p, p->dev, dev, p->table_bytes, p->rt.tab.data(), p->tile_pos(),
                       p->tile.data(), tab);
}

// ... and its packed-order table.
static int plan_packed(MPIX_Iov_plan_s *p, int dev, char **tab)
{
    return plan_upload(p, p->pk_dev, dev, p->pk.size(), p->pk.data(), p->pk.size(), nullptr, tab);
}

// MPIX_Iov_plan_prepare[_packed]: the device argument resolved, then `upload`.
static int plan_prepare(MPIX_Iov_plan plan, int device,
                        int (*upload)(MPIX_Iov_plan_s *, int, char **))
{
    if (!plan)
        return MPIX_REDOP_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void) hipGetLastError();
        return MPIX_REDOP_ERR_OTHER;
    }
    if (device == -1 && hipGetDevice(&device) != hipSuccess)
        return MPIX_REDOP_ERR_OTHER;
    if (device < 0 || device >= ndev)
        return MPIX_REDOP_ERR_ARG;
    char *tab;
    return upload(plan, device, &tab);
}

int MPIX_Iov_plan_prepare(MPIX_Iov_plan plan, int device)
{
    return set_err(plan_prepare(plan, device, plan_tables));
}

int MPIX_Iov_plan_prepare_packed(MPIX_Iov_plan plan, int device)
{
    return set_err(plan_prepare(plan, device, plan_packed));
}

int MPIX_Iov_plan_info_packed(MPIX_Iov_plan plan, MPIX_Aint *table_bytes)
{
    if (!plan)
        return set_err(MPIX_REDOP_ERR_ARG);
    if (table_bytes)
        *table_bytes = (MPIX_Aint) plan->pk.size();
    return set_err(MPIX_REDOP_SUCCESS);
}

int MPIX_Iov_plan_locate(MPIX_Iov_plan plan, MPIX_Aint packed_index, MPIX_Aint *byte_offset)
{
    if (!plan || !byte_offset)
        return set_err(MPIX_REDOP_ERR_ARG);
    if (packed_index < 0 || (uint64_t) packed_index >= plan->total)
        return set_err(MPIX_REDOP_ERR_COUNT);
    *byte_offset = (MPIX_Aint) plan->locate((uint64_t) packed_index);
    return set_err(MPIX_REDOP_SUCCESS);
}

int MPIX_Iov_plan_info(MPIX_Iov_plan plan, MPIX_Aint *elements, MPIX_Aint *runs, MPIX_Aint *groups,
                       MPIX_Aint *lo_byte, MPIX_Aint *hi_byte, MPIX_Aint *table_bytes)
{
    if (!plan)
        return set_err(MPIX_REDOP_ERR_ARG);
    if (elements)
        *elements = (MPIX_Aint) plan->total;
    if (runs)
        *runs = (MPIX_Aint) plan->nrun;
    if (groups)     // a single run is one group, though it has no table
        *groups = plan->nrun == 1 ? 1 : (MPIX_Aint) plan->groups();
    if (lo_byte)
        *lo_byte = (MPIX_Aint) plan->lo;
    if (hi_byte)
        *hi_byte = (MPIX_Aint) plan->hi;
    if (table_bytes)
        *table_bytes = (MPIX_Aint) plan->table_bytes;
    return set_err(MPIX_REDOP_SUCCESS);
}

int MPIX_Iov_plan_free(MPIX_Iov_plan *plan)
{
    if (!plan)
        return set_err(MPIX_REDOP_ERR_ARG);
    MPIX_Iov_plan_s *p = *plan;
    *plan = nullptr;
    if (!p)
        return set_err(MPIX_REDOP_SUCCESS);
    int rc = MPIX_REDOP_SUCCESS;
    for (int d = 0; d < kMaxDev; ++d) {
        for (char *t : {p->dev[d].load(std::memory_order_acquire),
                        p->pk_dev[d].load(std::memory_order_acquire)}) {
            if (!t)
                continue;
            DeviceGuard guard(d);
            const int rc2 = hip_err(hipFree(t));
            rc = rc ? rc : rc2;
        }
    }
    delete p;
    return set_err(rc);
}

// One side of a plan-taking call: its buffer, its plan (NULL: packed) and, from
// them, the bounding byte range the overlap check looks at and the base and
// table the kernels address it with.
struct TypedSide {
    const void *buf;
    MPIX_Iov_plan_s *plan;
    // (an operand the op does not read may be NULL: no pointer arithmetic on it)
    const void *lo() const
    {
        return (const void *) ((uintptr_t) buf + (uintptr_t) (plan ? plan->lo : 0));
    }
    uint64_t span(uint64_t packed) const
    {
        return plan ? (uint64_t) (plan->hi - plan->lo) : packed;
    }
    bool table() const { return plan && plan->nrun > 1; }
    int64_t one_off() const { return plan && plan->nrun == 1 ? plan->one_off : 0; }
};

// The device-free checks of the plan entries (1-6) and of the typed entries
// (1-7, mpix_redop.h): one list, the plan entries' sides being packed (no side
// plan).  reads_origin is the caller's rule (plan_run).  *n = 0 when there is
// nothing to do.
static int plan_validate(const TypedSide &o, const TypedSide &r, const void *target,
                         MPIX_Iov_plan_s *tp, uint32_t op, bool fetch, bool reads_origin,
                         uint64_t *n)
{
    *n = 0;
    if (!tp)
        return MPIX_REDOP_ERR_ARG;
    if (!is_builtin_op(op) || (op & 0xf) == kOpEqual || !internal_ok(op, tp->it))
        return MPIX_REDOP_ERR_OP;
    const uint32_t opi = op & 0xf;
    for (const MPIX_Iov_plan_s *q : {o.plan, r.plan}) {
        if (q && q->it != tp->it)
            return MPIX_REDOP_ERR_TYPE;
        if (q && q->total != tp->total)
            return MPIX_REDOP_ERR_COUNT;
    }
    if (tp->total == 0)
        return MPIX_REDOP_SUCCESS;
    if (missing_operand(o.buf, r.buf, target, fetch, reads_origin))
        return MPIX_REDOP_ERR_BUFFER;
    const uint64_t packed = tp->total * tp->ext;
    if (operands_overlap(o.lo(), o.span(packed), r.lo(), r.span(packed),
                         (const char *) target + tp->lo, (uint64_t) (tp->hi - tp->lo), fetch,
                         reads_origin))
        return MPIX_REDOP_ERR_BUFFER;
    // plan_entry answers for typed_entry, and for gpu_entry / getacc_entry, which
    // a plan of one run launches through: every family is built from the one
    // (type, op) table (redop_tables.h), so one lookup answers for all
    if (opi < kOpReplace && !plan_entry(opi, tp->it))
        return MPIX_REDOP_ERR_TYPE;     // a legal pair without a kernel
    *n = tp->total;
    return MPIX_REDOP_SUCCESS;
}

// Validated arguments: operand placement, the device's tables, the launches on
// `s` -- one per residue group of the target plan; with no table on any side,
// the contiguous entries' path with each buffer at its run's offset.  typed:
// the typed entries' kernels (k_typed_*), which take the sides' packed-order
// tables; else the plan entries' (k_plan_*), whose sides are packed.
static int plan_enqueue(const TypedSide &o, const TypedSide &r, void *target, MPIX_Iov_plan_s *tp,
                        uint32_t op, bool fetch, bool reads_origin, bool typed, hipStream_t s)
{
    const uint32_t opi = op & 0xf;
    Placed q{o.buf, r.buf, target};
    if (!place_operands(&q, fetch, false, reads_origin, s))
        return MPIX_REDOP_ERR_BUFFER;
    if (!fetch && opi == kOpNoOp)
        return MPIX_REDOP_SUCCESS;
    const bool otab = reads_origin && o.table(), rtab = fetch && r.table();
    const char *po = (const char *) q.origin + o.one_off();
    char *pr = (char *) q.result + r.one_off();
    if (tp->nrun == 1 && !otab && !rtab) {
        char *t1 = (char *) q.target + tp->one_off;
        if (!fetch)
            return enqueue(Combine{po, t1, tp->total, tp->it, tp->ext, op}, s, q.zc);
        return getacc_launch(po, pr, t1, tp->total, 1, 1, tp->it, tp->ext, opi, q.zc, s);
    }
    const bool copies = opi >= kOpReplace;      // MPI_REPLACE, MPI_NO_OP: the copy kernels
    const mpix::PlanEntry *pe = typed || copies ? nullptr : plan_entry(opi, tp->it);
    const mpix::TypedEntry *te = typed && !copies ? typed_entry(opi, tp->it) : nullptr;
    if (!copies && !pe && !te)
        return MPIX_REDOP_ERR_TYPE;
    const int dev = q.launch == -2 ? stream_device(s) : q.launch;
    char *tab = nullptr, *otb = nullptr, *rtb = nullptr;
    int rc = plan_tables(tp, dev, &tab);
    if (rc == MPIX_REDOP_SUCCESS && otab)
        rc = plan_packed(o.plan, dev, &otb);
    if (rc == MPIX_REDOP_SUCCESS && rtab)
        rc = plan_packed(r.plan, dev, &rtb);
    if (rc != MPIX_REDOP_SUCCESS)
        return rc;
    mpix::TypedRuns tr{nullptr, nullptr, 1, tp->total,
                       otab ? mpix::PackedTab(otb, o.plan->nrun) : mpix::PackedTab(),
                       rtab ? mpix::PackedTab(rtb, r.plan->nrun) : mpix::PackedTab()};
    PairMap pm{0, 0};
    (void) padded_pair(tp->it, &pm);
    const mpix::CopyMode mode = copy_mode(opi, fetch);
    const uint32_t ext = (uint32_t) tp->ext;
    auto launch = [&](void *tg) {
        if (typed && copies)
            return hip_err(mpix::launch_typed_copy(mode, ext, pm.value_bytes, pm.loc_off, po, pr, tg,
                                                   tr, launch_cfg(), s));
        if (typed)
            return hip_err(fetch ? te->getacc(po, pr, tg, tr, params(), launch_cfg(), s)
                                 : te->acc(po, tg, tr, params(), launch_cfg(), s));
        if (copies)
            return hip_err(mpix::launch_plan_copy(mode, ext, pm.value_bytes, pm.loc_off, po, pr, tg,
                                                  tr.d_tab, tr.d_tile, tr.nseg, tr.total,
                                                  launch_cfg(), s));
        return hip_err(fetch ? pe->getacc(po, pr, tg, tr.d_tab, tr.d_tile, tr.nseg, tr.total,
                                          params(), launch_cfg(), s)
                             : pe->reduce(po, tg, tr.d_tab, tr.d_tile, tr.nseg, tr.total, params(),
                                          launch_cfg(), s));
    };
    if (tp->nrun == 1)      // typed only: a side has a table
        return launch((char *) q.target + tp->one_off);
    return tp->each_group(tab, [&](const ResidueGroup &gr) {
        tr.d_tab = gr.seg_off;      // the group's whole table
        tr.d_tile = gr.tile;
        tr.nseg = gr.n;
        tr.total = gr.total;
        return launch((char *) q.target + gr.resid);
    });
}

// Every form of the plan entries (typed = false: origin and result packed, no
// side plan) and of the typed entries.  The origin is an operand unless the op
// is MPI_NO_OP -- for the plan entries only in their fetch form; the typed
// entries then look at neither origin nor origin_plan.
static int plan_run(const void *origin, MPIX_Iov_plan origin_plan, void *result,
                    MPIX_Iov_plan result_plan, void *target, MPIX_Iov_plan target_plan, uint32_t op,
                    bool fetch, bool typed, bool sync, hipStream_t stream)
{
    const bool noop = (op & 0xf) == kOpNoOp;
    const bool reads_origin = !(noop && (typed || fetch));
    const TypedSide o{typed && noop ? nullptr : origin, noop ? nullptr : origin_plan},
        r{result, result_plan};
    uint64_t n;
    int rc = plan_validate(o, r, target, target_plan, op, fetch, reads_origin, &n);
    if (rc != MPIX_REDOP_SUCCESS || n == 0)
        return rc;
    return on_stream(sync, stream, target, [&](hipStream_t s) {
        return plan_enqueue(o, r, target, target_plan, op, fetch, reads_origin, typed, s);
    });
}

int MPIX_Reduce_local_plan_async(const void *inbuf, void *inoutbuf, MPIX_Iov_plan plan, MPIX_Op op,
                                 void *stream)
{
    return set_err(plan_run(inbuf, nullptr, nullptr, nullptr, inoutbuf, plan, (uint32_t) op,
                            false, false, false, (hipStream_t) stream));
}

int MPIX_Reduce_local_plan(const void *inbuf, void *inoutbuf, MPIX_Iov_plan plan, MPIX_Op op)
{
    return set_err(plan_run(inbuf, nullptr, nullptr, nullptr, inoutbuf, plan, (uint32_t) op,
                            false, false, true, nullptr));
}

int MPIX_Get_accumulate_local_plan_async(const void *origin, void *result, void *target,
                                         MPIX_Iov_plan plan, MPIX_Op op, void *stream)
{
    return set_err(plan_run(origin, nullptr, result, nullptr, target, plan, (uint32_t) op, true,
                            false, false, (hipStream_t) stream));
}

int MPIX_Get_accumulate_local_plan(const void *origin, void *result, void *target,
                                   MPIX_Iov_plan plan, MPIX_Op op)
{
    return set_err(plan_run(origin, nullptr, result, nullptr, target, plan, (uint32_t) op, true,
                            false, true, nullptr));
}

// ------------------------------------- a datatype on every side
// MPIX_[Get_]accumulate_local_typed*: origin and result as plans too (NULL:
// packed); plan_run with typed = true.
int MPIX_Accumulate_local_typed_async(const void *origin, MPIX_Iov_plan origin_plan, void *target,
                                      MPIX_Iov_plan target_plan, MPIX_Op op, void *stream)
{
    return set_err(plan_run(origin, origin_plan, nullptr, nullptr, target, target_plan,
                            (uint32_t) op, false, true, false, (hipStream_t) stream));
}

int MPIX_Accumulate_local_typed(const void *origin, MPIX_Iov_plan origin_plan, void *target,
                                MPIX_Iov_plan target_plan, MPIX_Op op)
{
    return set_err(plan_run(origin, origin_plan, nullptr, nullptr, target, target_plan,
                            (uint32_t) op, false, true, true, nullptr));
}

int MPIX_Get_accumulate_local_typed_async(const void *origin, MPIX_Iov_plan origin_plan,
                                          void *result, MPIX_Iov_plan result_plan, void *target,
                                          MPIX_Iov_plan target_plan, MPIX_Op op, void *stream)
{
    return set_err(plan_run(origin, origin_plan, result, result_plan, target, target_plan,
                            (uint32_t) op, true, true, false, (hipStream_t) stream));
}

int MPIX_Get_accumulate_local_typed(const void *origin, MPIX_Iov_plan origin_plan, void *result,
                                    MPIX_Iov_plan result_plan, void *target,
                                    MPIX_Iov_plan target_plan, MPIX_Op op)
{
    return set_err(plan_run(origin, origin_plan, result, result_plan, target, target_plan,
                            (uint32_t) op, true, true, true, nullptr));
}

// ------------------------------------- element-atomic accumulate
// The counterpart of the reference handing an accumulate to hardware atomics
// where its (type, op) table allows (ofi_rma.h:67-132, MPIDI_OFI_query_acc_
// atomic_support): device-scope read-modify-write / compare-exchange per
// element on the word that holds it (redop_atomic.h).
static const mpix::AtomicEntry *atomic_entry(uint32_t opi, uint32_t it)
{
    return entry_of(mpix::lookup_acc_atomic_fp, mpix::lookup_acc_atomic_int,
                    mpix::lookup_acc_atomic_pair, opi, it);
}

static bool atomic_extent(uint64_t ext) { return ext == 1 || ext == 2 || ext == 4 || ext == 8; }

// MPIR_Type_is_rma_atomic (rmatypeutil.c:18-30): the integer group of
// internal types only
static bool rma_atomic_type(uint32_t it)
{
    if (it == kNull || !is_builtin(it) || !(it & 0x800000u) || (it & 0x400000u))
        return false;
    return integer_kind(it & 0x0f0000u);
}

// The pair alone, no HIP call: legal, a kernel in the table, and an extent
// the device has an atomic for.  MPI_OP_NULL asks about compare-and-swap.
static int atomic_supported(uint32_t op, uint32_t it)
{
    if (it == kNull || !atomic_extent(extent_of(it)))
        return 0;
    if (op == kOpNull)
        return rma_atomic_type(it) ? 1 : 0;
    if (!is_builtin_op(op) || (op & 0xf) == kOpEqual || !internal_ok(op, it))
        return 0;
    const uint32_t opi = op & 0xf;
    if (opi == kOpReplace || opi == kOpNoOp)
        return 1;
    const mpix::AtomicEntry *e = atomic_entry(opi, it);
    return (e && e->acc && e->getacc) ? 1 : 0;
}

// getacc_validate's checks in its order for a contiguous target (fetch: the
// call has a result), then the two of this family: a pair without an atomic
// kernel (MPI_ERR_TYPE) and a target not aligned to its extent
// (MPI_ERR_BUFFER).  No device work.
static int atomic_validate(const void *origin, const void *result, const void *target,
                           MPIX_Aint count, uint32_t dt, uint32_t op, bool fetch, uint32_t *it,
                           uint64_t *ext, uint64_t *n)
{
    *n = 0;
    if (count < 0)
        return MPIX_REDOP_ERR_COUNT;
    if (is_builtin_op(op) && (op & 0xf) == kOpEqual)
        return MPIX_REDOP_ERR_OP;       // MPIX_EQUAL is no accumulate op
    int rc = validate(nullptr, nullptr, 0, dt, op, it, ext);
    if (rc != MPIX_REDOP_SUCCESS || count == 0)
        return rc;
    const uint64_t c = (uint64_t) count;
    if (c > ((uint64_t) 1 << 56) / *ext)
        return MPIX_REDOP_ERR_COUNT;
    const bool reads_origin = (op & 0xf) != kOpNoOp;    // with or without a result
    if (missing_operand(origin, result, target, fetch, reads_origin))
        return MPIX_REDOP_ERR_BUFFER;
    if (operands_overlap(origin, result, target, c * *ext, c * *ext, fetch, reads_origin))
        return MPIX_REDOP_ERR_BUFFER;
    if (!atomic_supported(op, *it))
        return MPIX_REDOP_ERR_TYPE;     // no kernel, or no atomic of this extent
    if ((uintptr_t) target % *ext)
        return MPIX_REDOP_ERR_BUFFER;   // the element would straddle its word
    *n = c;
    return MPIX_REDOP_SUCCESS;
}

// Device-scope atomics cover device memory of the launching device only: not
// page-locked host memory, not managed memory, not a peer's.
static bool atomic_target_ok(const void *target, int dev)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, target) != hipSuccess) {
        (void) hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice && a.device == dev;
}

static int atomic_enqueue(const void *origin, void *result, void *target, uint64_t count,
                          uint32_t it, uint64_t ext, uint32_t op, bool fetch, hipStream_t s)
{
    const uint32_t opi = op & 0xf;
    Placed p{origin, result, target, stream_device(s)};
    if (!atomic_target_ok(target, p.launch) || !place_operands(&p, fetch, true, opi != kOpNoOp, s))
        return MPIX_REDOP_ERR_BUFFER;
    if (opi == kOpNoOp && !fetch)
        return MPIX_REDOP_SUCCESS;
    const LaunchCfg cfg = launch_cfg(p.zc);
    if (opi == kOpReplace || opi == kOpNoOp) {
        PairMap pm{0, 0};
        (void) padded_pair(it, &pm);
        return hip_err(mpix::launch_atomic_copy(copy_mode(opi, fetch), (uint32_t) ext,
                                                pm.value_bytes, pm.loc_off, p.origin,
                                                (void *) p.result, target, count, cfg, s));
    }
    const mpix::AtomicEntry *e = atomic_entry(opi, it);
    if (!e || !e->acc || !e->getacc)
        return MPIX_REDOP_ERR_TYPE;
    if (fetch)
        return hip_err(e->getacc(p.origin, (void *) p.result, target, count, params(), cfg, s));
    return hip_err(e->acc(p.origin, target, count, params(), cfg, s));
}

// Either form of the accumulate (fetch = false, no result) and the fetch entry.
static int atomic_run(const void *origin, void *result, void *target, MPIX_Aint count, uint32_t dt,
                      uint32_t op, bool fetch, bool sync, hipStream_t stream)
{
    uint32_t it;
    uint64_t ext, n;
    int rc = atomic_validate(origin, result, target, count, dt, op, fetch, &it, &ext, &n);
    if (rc != MPIX_REDOP_SUCCESS || n == 0)
        return rc;
    return on_stream(sync, stream, target, [&](hipStream_t s) {
        return atomic_enqueue(origin, result, target, n, it, ext, op, fetch, s);
    });
}

int MPIX_Accumulate_local_atomic_async(const void *origin, void *target, MPIX_Aint count,
                                       MPIX_Datatype datatype, MPIX_Op op, void *stream)
{
    return set_err(atomic_run(origin, nullptr, target, count, (uint32_t) datatype, (uint32_t) op,
                              false, false, (hipStream_t) stream));
}

int MPIX_Accumulate_local_atomic(const void *origin, void *target, MPIX_Aint count,
                                 MPIX_Datatype datatype, MPIX_Op op)
{
    return set_err(atomic_run(origin, nullptr, target, count, (uint32_t) datatype, (uint32_t) op,
                              false, true, nullptr));
}

int MPIX_Get_accumulate_local_atomic_async(const void *origin, void *result, void *target,
                                           MPIX_Aint count, MPIX_Datatype datatype, MPIX_Op op,
                                           void *stream)
{
    return set_err(atomic_run(origin, result, target, count, (uint32_t) datatype, (uint32_t) op,
                              true, false, (hipStream_t) stream));
}

int MPIX_Get_accumulate_local_atomic(const void *origin, void *result, void *target,
                                     MPIX_Aint count, MPIX_Datatype datatype, MPIX_Op op)
{
    return set_err(atomic_run(origin, result, target, count, (uint32_t) datatype, (uint32_t) op,
                              true, true, nullptr));
}

// ------------------------------------- compare-and-swap
// MPI_Compare_and_swap's local step on one element of an RMA-atomic type, as
// a one-thread kernel or (atomic) as one device-scope compare-exchange.  The
// atomic form's two checks come last: no 16-byte atomic (MPI_ERR_TYPE), a
// target aligned to its size (MPI_ERR_BUFFER).
static int cas_validate(const void *origin, const void *compare, const void *result,
                        const void *target, uint32_t dt, bool atomic, uint32_t *size)
{
    const uint32_t it = to_internal(dt);
    const uint64_t ext = extent_of(it);
    if (!rma_atomic_type(it) || (!atomic_extent(ext) && ext != 16))
        return MPIX_REDOP_ERR_TYPE;
    if (no_buffer(origin) || no_buffer(compare) || no_buffer(result) || no_buffer(target))
        return MPIX_REDOP_ERR_BUFFER;
    // origin and compare are both only read: they may share an address
    if (ranges_overlap(result, ext, origin, ext) || ranges_overlap(result, ext, compare, ext) ||
        ranges_overlap(result, ext, target, ext) || ranges_overlap(target, ext, origin, ext) ||
        ranges_overlap(target, ext, compare, ext))
        return MPIX_REDOP_ERR_BUFFER;
    if (atomic && !atomic_extent(ext))
        return MPIX_REDOP_ERR_TYPE;
    if (atomic && (uintptr_t) target % ext)
        return MPIX_REDOP_ERR_BUFFER;
    *size = (uint32_t) ext;
    return MPIX_REDOP_SUCCESS;
}

// Placement -- the atomic form's target by atomic_target_ok, first; otherwise
// origin, compare, result, target -- and the launch.
static int cas_enqueue(const void *origin, const void *compare, void *result, void *target,
                       uint32_t size, bool atomic, hipStream_t s)
{
    const void *po, *pc, *pr, *pt = target;
    int launch = -2;
    if (atomic && !atomic_target_ok(target, launch = stream_device(s)))
        return MPIX_REDOP_ERR_BUFFER;
    if (!reachable(origin, s, &launch, &po) || !reachable(compare, s, &launch, &pc) ||
        !reachable(result, s, &launch, &pr) || (!atomic && !reachable(target, s, &launch, &pt)))
        return MPIX_REDOP_ERR_BUFFER;
    return hip_err((atomic ? mpix::launch_cas_atomic : mpix::launch_cas)(size, po, pc, (void *) pr,
                                                                         (void *) pt, s));
}

static int cas_run(const void *origin, const void *compare, void *result, void *target,
                   uint32_t dt, bool atomic, bool sync, hipStream_t stream)
{
    uint32_t size;
    int rc = cas_validate(origin, compare, result, target, dt, atomic, &size);
    if (rc != MPIX_REDOP_SUCCESS)
        return rc;
    return on_stream(sync, stream, target, [&](hipStream_t s) {
        return cas_enqueue(origin, compare, result, target, size, atomic, s);
    });
}

int MPIX_Compare_and_swap_local_async(const void *origin, const void *compare, void *result,
                                      void *target, MPIX_Datatype datatype, void *stream)
{
    return set_err(cas_run(origin, compare, result, target, (uint32_t) datatype, false, false,
                           (hipStream_t) stream));
}

int MPIX_Compare_and_swap_local(const void *origin, const void *compare, void *result,
                                void *target, MPIX_Datatype datatype)
{
    return set_err(cas_run(origin, compare, result, target, (uint32_t) datatype, false, true,
                           nullptr));
}

int MPIX_Compare_and_swap_local_atomic_async(const void *origin, const void *compare, void *result,
                                             void *target, MPIX_Datatype datatype, void *stream)
{
    return set_err(cas_run(origin, compare, result, target, (uint32_t) datatype, true, false,
                           (hipStream_t) stream));
}

int MPIX_Compare_and_swap_local_atomic(const void *origin, const void *compare, void *result,
                                       void *target, MPIX_Datatype datatype)
{
    return set_err(cas_run(origin, compare, result, target, (uint32_t) datatype, true, true,
                           nullptr));
}

int MPIX_Accumulate_atomic_is_supported(MPIX_Op op, MPIX_Datatype datatype)
{
    return atomic_supported((uint32_t) op, to_internal((uint32_t) datatype));
}

int MPIX_Reduce_local_multi_async(const void *const *inbufs, int ninputs, void *inoutbuf,
                                  MPIX_Aint count, MPIX_Datatype datatype, MPIX_Op op,
                                  void *stream)
{
    if (ninputs < 1 || ninputs > mpix::kMaxMultiInputs || !inbufs)
        return set_err(MPIX_REDOP_ERR_ARG);
    uint32_t it;
    uint64_t ext;
    for (int q = 0; q < ninputs; ++q) {
        int rc = validate(inbufs[q], inoutbuf, count, (uint32_t) datatype, (uint32_t) op, &it,
                          &ext);
        if (rc != MPIX_REDOP_SUCCESS)
            return set_err(rc);
    }
    if (count == 0)
        return set_err(MPIX_REDOP_SUCCESS);
    const void *dins[mpix::kMaxMultiInputs];
    const void *pio;
    int launch = -2;
    if (!reachable(inoutbuf, (hipStream_t) stream, &launch, &pio))
        return set_err(MPIX_REDOP_ERR_BUFFER);
    for (int q = 0; q < ninputs; ++q)
        if (!reachable(inbufs[q], (hipStream_t) stream, &launch, &dins[q]))
            return set_err(MPIX_REDOP_ERR_BUFFER);
    inbufs = dins;
    inoutbuf = (void *) pio;
    uint32_t opi = (uint32_t) op & 0xf;
    if (opi == kOpNoOp)
        return set_err(MPIX_REDOP_SUCCESS);
    if (opi == kOpReplace)      // REPLACE k times = copy of the last input
        return set_err(replace_rows(inoutbuf, ext, inbufs[ninputs - 1], ext, (uint64_t) count, it,
                                    ext, (hipStream_t) stream));
    const Entry *e = gpu_entry(opi, it);
    if (!e)
        return set_err(MPIX_REDOP_ERR_TYPE);
    return set_err(hip_err(e->multi(inbufs, ninputs, inoutbuf, (uint64_t) count, params(),
                                    launch_cfg(), (hipStream_t) stream)));
}

int MPIX_Reduce_local_tree_async(const void *const *inbufs, int ninputs, void *outbuf,
                                 MPIX_Aint count, MPIX_Datatype datatype, MPIX_Op op, void *stream)
{
    if (ninputs < 2 || ninputs > mpix::kMaxMultiInputs || (ninputs & (ninputs - 1)) || !inbufs ||
        !inbufs[0])
        return set_err(MPIX_REDOP_ERR_ARG);
    uint32_t it;
    uint64_t ext;
    // outbuf may be one of the slots itself; any partial overlap is refused.
    // What makes that safe: the tree kernels read all their slots' elements
    // of a unit before they write that unit, and a unit is one lane's alone.
    // The two-launch split combiners on the 32-byte route do not (k_contig32
    // stores the inout role's value into a unit it declines and k_fixup32
    // reads both operands again): there out over slot 0 is safe because slot 0
    // is that role, and out over slot 1 goes to the element kernel
    // (launch_tree).  Slots 1..k-1 may be NULL: absent (the partner passes
    // through).
    for (int q = 0; q < ninputs; ++q) {
        if (!inbufs[q])
            continue;
        const bool same = inbufs[q] == (const void *) outbuf;
        int rc = validate(same ? (const void *) ((const char *) outbuf + 1) : inbufs[q], outbuf,
                          same ? 0 : count, (uint32_t) datatype, (uint32_t) op, &it, &ext);
        if (rc == MPIX_REDOP_SUCCESS && same && count > 0 &&
            (uint64_t) count > ((uint64_t) 1 << 56) / ext)
            rc = MPIX_REDOP_ERR_COUNT;
        if (rc == MPIX_REDOP_SUCCESS && same && count > 0 &&
            no_buffer(outbuf))
            rc = MPIX_REDOP_ERR_BUFFER;
        if (rc != MPIX_REDOP_SUCCESS)
            return set_err(rc);
    }
    if (count == 0)
        return set_err(MPIX_REDOP_SUCCESS);
    uint32_t opi = (uint32_t) op & 0xf;
    if (opi == kOpEqual)
        return set_err(MPIX_REDOP_ERR_OP);      // EQUAL is never split or folded
    const void *dins[mpix::kMaxMultiInputs];
    const void *pout;
    int launch = -2;
    if (!reachable(outbuf, (hipStream_t) stream, &launch, &pout))
        return set_err(MPIX_REDOP_ERR_BUFFER);
    int last = 0;
    for (int q = 0; q < ninputs; ++q) {
        dins[q] = nullptr;
        if (inbufs[q] && !reachable(inbufs[q], (hipStream_t) stream, &launch, &dins[q]))
            return set_err(MPIX_REDOP_ERR_BUFFER);
        if (inbufs[q])
            last = q;
    }
    if (opi == kOpReplace || opi == kOpNoOp) {  // fold to the last present slot / to the first
        const void *src = dins[opi == kOpReplace ? last : 0];
        if (src == pout)
            return set_err(MPIX_REDOP_SUCCESS);
        return set_err(replace_rows((void *) pout, ext, src, ext, (uint64_t) count, it, ext,
                                    (hipStream_t) stream));
    }
    const Entry *e = gpu_entry(opi, it);
    if (!e || !e->tree)
        return set_err(MPIX_REDOP_ERR_TYPE);
    return set_err(hip_err(e->tree(dins, ninputs, (void *) pout, (uint64_t) count, params(),
                                   launch_cfg(), (hipStream_t) stream)));
}

int MPIX_Copy_multi_async(const void *const *srcs, void *const *dsts, const MPIX_Aint *bytes,
                          int n, void *stream)
{
    if (n < 0 || n > mpix::kMaxMultiInputs || (n && (!srcs || !dsts || !bytes)))
        return set_err(MPIX_REDOP_ERR_ARG);
    const void *ds[mpix::kMaxMultiInputs];
    void *dd[mpix::kMaxMultiInputs];
    uint64_t nb[mpix::kMaxMultiInputs];
    int m = 0, launch = -2;
    for (int q = 0; q < n; ++q) {
        if (bytes[q] < 0)
            return set_err(MPIX_REDOP_ERR_COUNT);
        if (bytes[q] == 0)
            continue;
        if (!srcs[q] || !dsts[q] || overlaps(srcs[q], dsts[q], (uint64_t) bytes[q]))
            return set_err(MPIX_REDOP_ERR_BUFFER);
        const void *pd;
        if (!reachable(srcs[q], (hipStream_t) stream, &launch, &ds[m]) ||
            !reachable(dsts[q], (hipStream_t) stream, &launch, &pd))
            return set_err(MPIX_REDOP_ERR_BUFFER);
        dd[m] = (void *) pd;
        nb[m++] = (uint64_t) bytes[q];
    }
    if (!m)
        return set_err(MPIX_REDOP_SUCCESS);
    launch_cfg();
    return set_err(hip_err(mpix::launch_copy_multi(ds, dd, nb, m, (hipStream_t) stream,
                                                   (unsigned) launch_cfg().wt_xcd)));
}

int MPIX_Ipc_export(const void *devptr, void *handle_out, MPIX_Aint *offset_out)
{
    if (!devptr || !handle_out || !offset_out)
        return set_err(MPIX_REDOP_ERR_ARG);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    hipError_t e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t) devptr);
    if (e != hipSuccess)
        return set_err(hip_err(e));
    hipIpcMemHandle_t h;
    e = hipIpcGetMemHandle(&h, (void *) base);
    if (e != hipSuccess)
        return set_err(hip_err(e));
    memcpy(handle_out, &h, sizeof(h));
    *offset_out = (MPIX_Aint) ((const char *) devptr - (const char *) base);
    return set_err(MPIX_REDOP_SUCCESS);
}

int MPIX_Ipc_open(const void *handle, void **base_out)
{
    if (!handle || !base_out)
        return set_err(MPIX_REDOP_ERR_ARG);
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    return set_err(hip_err(hipIpcOpenMemHandle(base_out, h, hipIpcMemLazyEnablePeerAccess)));
}

int MPIX_Ipc_close(void *base)
{
    return set_err(hip_err(hipIpcCloseMemHandle(base)));
}

int MPIX_Redop_peer_access(int device, int peer_device)
{
    return peer_access(device, peer_device) ? 1 : 0;
}

// the (op, type) half of the predicate: a kernel exists (knob-independent)
static int has_gpu_path(uint32_t op, uint32_t it)
{
    if (it == kNull || extent_of(it) == 0 || !internal_ok(op, it))
        return 0;
    uint32_t opi = op & 0xf;
    if (opi == kOpReplace || opi == kOpNoOp)
        return 1;
    if (opi == kOpEqual)
        return (it & 0xffffff00u) == U8;
    return gpu_entry(opi, it) ? 1 : 0;
}

int MPIX_Redop_has_gpu_path(MPIX_Op op, MPIX_Datatype datatype)
{
    return has_gpu_path((uint32_t) op, to_internal((uint32_t) datatype));
}

// MPIR_Typerep_reduce_is_supported (typerep_yaksa_pack.c:227-271): the enable
// knob, the size threshold on the packed size for count > 0 (count 0, as
// reduce_local.c:68 passes it, only asks about the pair), then the pair
int MPIX_Redop_is_supported(MPIX_Op op, MPIX_Aint count, MPIX_Datatype datatype)
{
    env();
    if (!g_enable.load())
        return 0;
    uint32_t it = to_internal((uint32_t) datatype);
    if (count > 0) {
        const long long thr = g_threshold.load();
        const uint64_t sz = size_of(it);
        if (thr > 0 && sz && (uint64_t) count > (uint64_t) thr / sz)
            return 0;
    }
    return has_gpu_path((uint32_t) op, it);
}

// The same with the operands in view: both host-resident below the floor of
// their memory kind -> 0, MPICH keeps its op_fns.c loop for the chunk.  A
// device operand always goes to the GPU (the CPU could only reach it through
// two PCIe copies).
int MPIX_Redop_is_supported_buffers(MPIX_Op op, MPIX_Aint count, MPIX_Datatype datatype,
                                    const void *inbuf, const void *inoutbuf)
{
    if (!MPIX_Redop_is_supported(op, count, datatype))
        return 0;
    if (count <= 0 || !inbuf || !inoutbuf)
        return 1;
    int d0 = 0, d1 = 0;
    const void *p0, *p1;
    const Where w0 = classify(inbuf, &d0, &p0), w1 = classify(inoutbuf, &d1, &p1);
    if (w0 == Where::Device || w1 == Where::Device)
        return 1;
    const long long floor_bytes = (w0 == Where::Pageable || w1 == Where::Pageable)
                                      ? g_host_floor.load() : g_pinned_floor.load();
    const uint64_t bytes = (uint64_t) count * extent_of(to_internal((uint32_t) datatype));
    return (floor_bytes > 0 && bytes < (uint64_t) floor_bytes) ? 0 : 1;
}

int MPIX_Redop_set_support(int enable, MPIX_Aint threshold_bytes, MPIX_Aint host_floor_bytes,
                           MPIX_Aint pinned_floor_bytes)
{
    env();
    g_enable = enable != 0;
    g_threshold = (long long) threshold_bytes;
    g_host_floor = (long long) host_floor_bytes;
    g_pinned_floor = (long long) pinned_floor_bytes;
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_get_support(int *enable, MPIX_Aint *threshold_bytes, MPIX_Aint *host_floor_bytes,
                           MPIX_Aint *pinned_floor_bytes)
{
    env();
    if (enable)
        *enable = g_enable.load() ? 1 : 0;
    if (threshold_bytes)
        *threshold_bytes = (MPIX_Aint) g_threshold.load();
    if (host_floor_bytes)
        *host_floor_bytes = (MPIX_Aint) g_host_floor.load();
    if (pinned_floor_bytes)
        *pinned_floor_bytes = (MPIX_Aint) g_pinned_floor.load();
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_op_dt_check(MPIX_Op op, MPIX_Datatype datatype)
{
    return binding_ok((uint32_t) op, (uint32_t) datatype) ? 1 : 0;
}

int MPIX_Redop_internal_op_dt_check(MPIX_Op op, MPIX_Datatype datatype)
{
    return internal_ok((uint32_t) op, (uint32_t) datatype) ? 1 : 0;
}

MPIX_Datatype MPIX_Datatype_internal(MPIX_Datatype datatype)
{
    return (MPIX_Datatype) to_internal((uint32_t) datatype);
}

MPIX_Aint MPIX_Datatype_extent(MPIX_Datatype datatype)
{
    return (MPIX_Aint) extent_of(to_internal((uint32_t) datatype));
}

MPIX_Aint MPIX_Datatype_size(MPIX_Datatype datatype)
{
    return (MPIX_Aint) size_of(to_internal((uint32_t) datatype));
}

int MPIX_Redop_set_fortran_booleans(int true_value, int false_value)
{
    g_ftrue = true_value;
    g_ffalse = false_value;
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_set_launch(int block_threads, int max_grid)
{
    env();
    if (block_threads < 64 || block_threads > 1024 || block_threads % 64 || max_grid < 0)
        return MPIX_REDOP_ERR_ARG;
    g_block = block_threads;
    g_max_grid = max_grid;
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_set_store_policy(int xcd_mask, int every, int phase, int tail_blocks)
{
    env();
    if (xcd_mask < kWtAuto || xcd_mask > 0xff || every < 0 || phase < 0 ||
        phase >= (every > 0 ? every : 1) || tail_blocks < 0)
        return MPIX_REDOP_ERR_ARG;
    g_wt_xcd = xcd_mask;
    g_wt_every = every;
    g_wt_phase = phase;
    g_wt_tail = tail_blocks;
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_set_sync_store_policy(int xcd_mask)
{
    env();
    if (xcd_mask < kWtAuto || xcd_mask > 0xff)
        return MPIX_REDOP_ERR_ARG;
    g_wt_xcd_sync = xcd_mask;
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_get_sync_store_policy(int *xcd_mask)
{
    env();
    if (!xcd_mask)
        return MPIX_REDOP_ERR_ARG;
    // as launch_cfg(…, sync = true) resolves it; -1 while the default is
    // not settled (no launch so far)
    const int ws = g_wt_xcd_sync.load(), x = g_wt_xcd.load();
    *xcd_mask = ws != kWtAuto ? ws : x != kWtAuto ? x : g_wt_sync_default.load();
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_sync_timing(int device, int ncalls)
{
    env();
    if (device < 0 || device >= kMaxDev || ncalls < 0 || ncalls > kSyncTimingMax)
        return set_err(MPIX_REDOP_ERR_ARG);
    DeviceGuard g(device);
    DevState *d = dev_state(device);
    if (!d)
        return set_err(MPIX_REDOP_ERR_OTHER);
    while (d->tev.size() < 2 * (size_t) ncalls) {
        hipEvent_t e = nullptr;
        int rc = hip_err(hipEventCreate(&e));
        if (rc)
            return set_err(rc);
        d->tev.push_back(e);
    }
    d->t_cap = ncalls;
    d->t_used = 0;
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_sync_timing_read(int device, float *ms, int cap, int *got)
{
    env();
    if (device < 0 || device >= kMaxDev || !got || cap < 0 || (cap > 0 && !ms))
        return set_err(MPIX_REDOP_ERR_ARG);
    DeviceGuard g(device);
    DevState *d = dev_state(device);
    if (!d)
        return set_err(MPIX_REDOP_ERR_OTHER);
    const int n = d->t_used < cap ? d->t_used : cap;
    for (int i = 0; i < n; ++i) {
        int rc = hip_err(hipEventSynchronize(d->tev[2 * i + 1]));
        if (!rc)
            rc = hip_err(hipEventElapsedTime(&ms[i], d->tev[2 * i], d->tev[2 * i + 1]));
        if (rc)
            return set_err(rc);
    }
    *got = n;
    d->t_cap = d->t_used = 0;
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_get_store_policy(int *xcd_mask, int *every, int *phase, int *tail_blocks)
{
    env();
    if (xcd_mask) {     // -1: the default, not settled yet (no launch so far)
        const int x = g_wt_xcd.load();
        *xcd_mask = x == kWtAuto ? g_wt_default.load() : x;
    }
    if (every)
        *every = g_wt_every.load();
    if (phase)
        *phase = g_wt_phase.load();
    if (tail_blocks)
        *tail_blocks = g_wt_tail.load();
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_set_pageable(int threads, MPIX_Aint chunk_bytes)
{
    env();
    if (threads < 0 || threads > 16 || chunk_bytes < 65536 || chunk_bytes > ((MPIX_Aint) 256 << 20))
        return MPIX_REDOP_ERR_ARG;
    g_pipe_threads = threads;
    g_pipe_chunk = (size_t) chunk_bytes;
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_get_pageable(int *threads, MPIX_Aint *chunk_bytes)
{
    env();
    if (threads)
        *threads = g_pipe_threads.load();
    if (chunk_bytes)
        *chunk_bytes = (MPIX_Aint) g_pipe_chunk.load();
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_get_launch(int *block_threads, int *unroll, int *max_grid)
{
    env();
    if (block_threads)
        *block_threads = g_block.load();
    if (unroll)
        *unroll = mpix::unroll();
    if (max_grid)
        *max_grid = g_max_grid.load();
    return MPIX_REDOP_SUCCESS;
}

int MPIX_Redop_last_error(void) { return t_last_error; }

const char *MPIX_Redop_error_string(int code)
{
    switch (code) {
        case MPIX_REDOP_SUCCESS: return "success";
        case MPIX_REDOP_ERR_BUFFER: return "invalid buffer (NULL, MPI_IN_PLACE or aliased)";
        case MPIX_REDOP_ERR_COUNT: return "invalid count";
        case MPIX_REDOP_ERR_TYPE: return "datatype unknown or not supported on the GPU path";
        case MPIX_REDOP_ERR_OP: return "operation not defined for this datatype";
        case MPIX_REDOP_ERR_ARG: return "invalid argument";
        case MPIX_REDOP_ERR_OTHER: return "HIP runtime error";
        default: return "internal error";
    }
}

const char *MPIX_Redop_build_info(void)
{
#define MPIX_STR2(x) #x
#define MPIX_STR(x) MPIX_STR2(x)
    return mpix_build_info();
}

// ------------------------------------------------ MPIR_op_function table
// A failed call is fatal, like the reference's MPIR_Assert(0) on a type its
// op function does not cover (op_fns.c:51-53), unless MPIX_REDOP_OPFN_ABORT=0:
// then the error class is only recorded for MPIX_Redop_last_error().
static void opfn_failed(const char *name, int rc, MPIX_Datatype type)
{
    if (!g_opfn_abort.load())
        return;
    fprintf(stderr, "MPIX_Op_table: %s on datatype 0x%08x failed: %s (MPI error class %d); "
                    "only pairs MPIX_Redop_is_supported() accepts may use the table\n",
            name, (unsigned) type, MPIX_Redop_error_string(rc), rc);
    fflush(stderr);
    abort();
}
#define MPIX_OPFN(name, handle)                                                           \
    void name(void *invec, void *inoutvec, MPIX_Aint *len, MPIX_Datatype *type)           \
    {                                                                                     \
        env();          /* MPIX_REDOP_OPFN_ABORT, even if the call fails at once */      \
        int rc_ = MPIX_Reduce_local(invec, inoutvec, *len, *type, handle);               \
        if (rc_ != MPIX_REDOP_SUCCESS)                                                    \
            opfn_failed(#name, rc_, *type);                                               \
    }
MPIX_OPFN(MPIX_MAXF, MPIX_MAX)
MPIX_OPFN(MPIX_MINF, MPIX_MIN)
MPIX_OPFN(MPIX_SUM_fn, MPIX_SUM)
MPIX_OPFN(MPIX_PROD_fn, MPIX_PROD)
MPIX_OPFN(MPIX_LAND_fn, MPIX_LAND)
MPIX_OPFN(MPIX_BAND_fn, MPIX_BAND)
MPIX_OPFN(MPIX_LOR_fn, MPIX_LOR)
MPIX_OPFN(MPIX_BOR_fn, MPIX_BOR)
MPIX_OPFN(MPIX_LXOR_fn, MPIX_LXOR)
MPIX_OPFN(MPIX_BXOR_fn, MPIX_BXOR)
MPIX_OPFN(MPIX_MINLOC_fn, MPIX_MINLOC)
MPIX_OPFN(MPIX_MAXLOC_fn, MPIX_MAXLOC)
MPIX_OPFN(MPIX_REPLACE_fn, MPIX_REPLACE)
MPIX_OPFN(MPIX_NO_OP_fn, MPIX_NO_OP)
MPIX_OPFN(MPIX_EQUAL_fn, MPIX_EQUAL)
#undef MPIX_OPFN

// order of src/mpi/coll/op/oputil.c:10-27 / mpi.h.in:297-311
MPIX_op_function *const MPIX_Op_table[16] = {
    nullptr, MPIX_MAXF, MPIX_MINF, MPIX_SUM_fn, MPIX_PROD_fn, MPIX_LAND_fn, MPIX_BAND_fn,
    MPIX_LOR_fn, MPIX_BOR_fn, MPIX_LXOR_fn, MPIX_BXOR_fn, MPIX_MINLOC_fn, MPIX_MAXLOC_fn,
    MPIX_REPLACE_fn, MPIX_NO_OP_fn, MPIX_EQUAL_fn,
};

}  // extern "C"
