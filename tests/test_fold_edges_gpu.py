"""The multi-input fold (MPIX_Reduce_local_multi_async) and the tree fold
(MPIX_Reduce_local_tree_async) on the GPU: count edges, operands on different
16-byte phases, every presence mask, operand roles and launch settings.

Every case is held against two references:
  * the CPU oracle: oracle.reduce_local applied k times in order (multi) or
    level by level as tests/fold_model.py lays the tree out, under the parity
    rule of tests/test_gpu_parity.py (compare); padded pairs over the bytes of
    their type map only;
  * the single-call GPU path: the same sequence as MPIX_Reduce_local_async
    calls on device copies at the same byte offsets (a pass-through is a
    device copy).  The fold equals it bit for bit over the whole extent,
    padding and NaN payloads included -- "the same association, so the same
    bits" (redop_kernels.h).
and asserts return code 0, every input other than an in-place output
unchanged, and the guard bytes around every operand intact.

Kernels by launch condition (launch_multi / launch_tree): operands of a unit
of at most 16 bytes that share the output's 16-byte phase run the packet
kernels (k_contig_multi; k_contig_tree_rec<2,2> at k = 2, k_contig_tree<4,2>
at 4, k_contig_tree_rec<8,1> at 8, <16,1> at 16), any other placement and
every 32-byte unit the element kernels (k_elem_multi, k_elem_tree) -- but for
the two-slot tree of 32-byte units with both slots present and all three
operands on the 16-byte grid, which runs k_contig32 (tests/test_soft_fp_gpu.py
test_two_slot_tree_output_placement)."""
import types

import numpy as np
import pytest
import torch

from tests import fold_model as M
from tests.test_getacc_gpu import CANARY, GUARD, Placed, _soft_operands, field_mask
from tests.test_gpu_parity import SWEEP, _special_f64, compare, make_operand

pytestmark = pytest.mark.gpu

KINDS = {(s[0], s[1]): (s[2], s[3]) for s in SWEEP}
KINDS.update({('MPI_FLOAT', 'MPI_REPLACE'): ('fp', 4), ('MPI_FLOAT', 'MPI_NO_OP'): ('fp', 4),
              # 32-byte units: bit for bit against the oracle
              ('MPI_LONG_DOUBLE_INT', 'MPI_MAXLOC'): ('int', 32),
              ('MPI_COMPLEX32', 'MPI_PROD'): ('int', 32),
              ('MPI_COMPLEX32', 'MPI_SUM'): ('int', 32),
              ('MPI_C_LONG_DOUBLE_COMPLEX', 'MPI_PROD'): ('int', 32)})


@pytest.fixture(scope='module')
def R():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from mpich_amd import redop
    assert redop.lib().MPIX_Redop_init() == 0
    return redop


@pytest.fixture(scope='module')
def H():
    from mpich_amd import handles
    return handles


def ty(R, H, dtname, opname):
    kind, size = KINDS[(dtname, opname)]
    dt, op = getattr(H, dtname), getattr(H, opname)
    ext = R.datatype_extent(dt)
    return types.SimpleNamespace(dtname=dtname, opname=opname, dt=dt, op=op, ext=ext, kind=kind,
                                 size=size, E=max(1, 16 // ext), fields=field_mask(H, dt, ext))


def place(data, off):
    p = Placed(data, off)
    p.off = off
    return p


def device_copy(p):
    """a second buffer with p's bytes as they are on the device, at p's byte offset"""
    q = place(np.zeros(p.nb, np.uint8), p.off)
    q.v.copy_(p.v)
    return q


def read(p, what):
    """p's bytes, its guard bytes checked on the way"""
    h = p.buf.cpu().numpy()
    assert (h[:p.lo] == GUARD).all() and (h[p.lo + p.nb:] == GUARD).all(), ('guard bytes', what)
    return h[p.lo:p.lo + p.nb]


def oracle_mismatches(t, got, exp):
    if not t.fields.all():      # a padded pair: the bytes of its type map only
        got, exp = got.reshape(-1, t.ext).copy(), exp.reshape(-1, t.ext).copy()
        got[:, ~t.fields] = 0
        exp[:, ~t.fields] = 0
        got, exp = got.reshape(-1), exp.reshape(-1)
    return compare(got, exp, t.kind, t.size, t.opname, t.ext)


def counts_of(*cs):
    out = []
    for c in cs:
        if c > 0 and c not in out:
            out.append(c)
    return out


def seed(*parts):
    h = 0x5EED0F00
    for p in parts:
        for ch in str(p):
            h = (h * 131 + ord(ch)) & 0xffffffff
    return h


# ------------------------------------------------------------ multi fold
def multi_oracle(oracle, t, n, io, ins):
    exp = io[:n * t.ext].copy()
    for x in ins:
        assert oracle.reduce_local(x[:n * t.ext].copy(), exp, n, t.dt, t.op) == 0
    return exp


def check_multi(R, t, n, io, ins, io_off, in_offs, exp, ctx):
    """one multi-input fold of the first n elements of io and ins, placed at
    the given byte offsets; exp = the oracle's fold (its first n elements are
    used: every operation is element-wise)"""
    nb = n * t.ext
    io, ins = io[:nb], [x[:nb] for x in ins]
    T, T2 = place(io, io_off), place(io, io_off)
    ins_d = [place(x, o) for x, o in zip(ins, in_offs)]
    torch.cuda.synchronize()
    assert R.reduce_local_multi_async([p.v for p in ins_d], T.v, n, t.dt, t.op) == 0, ctx
    for p in ins_d:
        assert R.reduce_local_async(p.v, T2.v, n, t.dt, t.op) == 0, ctx
    got, ref = read(T, ctx), read(T2, ctx)
    for q, p in enumerate(ins_d):
        assert np.array_equal(read(p, ctx), ins[q]), ('input changed', q, ctx)
    assert np.array_equal(got, ref), ('differs from the single calls', ctx)
    assert oracle_mismatches(t, got, exp[:nb]) == 0, ('oracle', ctx)
    return got


EDGE_TYPES = [('MPI_FLOAT', 'MPI_SUM'), ('MPI_INT8_T', 'MPI_MAX'), ('MPI_UINT8_T', 'MPI_LXOR'),
              ('MPI_INT16_T', 'MPI_BXOR'), ('MPI_DOUBLE', 'MPI_PROD'), ('MPI_INTEGER16', 'MPI_SUM'),
              ('MPI_C_FLOAT_COMPLEX', 'MPI_PROD'), ('MPIR_2INT8', 'MPI_MINLOC'),
              ('MPI_SHORT_INT', 'MPI_MINLOC'), ('MPI_DOUBLE_INT', 'MPI_MAXLOC')]
EDGE_IDS = ['%s-%s' % e for e in EDGE_TYPES]


def multi_operands(t, n, k, *salt):
    """inout and k inputs of n elements (padded pairs: random padding bytes)"""
    rng = np.random.default_rng(seed(t.dtname, t.opname, *salt))
    return [make_operand(rng, t.kind, t.size, n, t.dtname) for _ in range(k + 1)]


@pytest.mark.parametrize('k', [1, 2, 3, 16])
@pytest.mark.parametrize('dtname,opname', EDGE_TYPES, ids=EDGE_IDS)
def test_multi_packet_edges(R, H, oracle, dtname, opname, k):
    """A1, k_contig_multi: every operand on the inout's phase; counts below
    the head, without a packet, of one packet, one block's tile and a packet
    either side, two tiles and a tail"""
    t = ty(R, H, dtname, opname)
    E, B = t.E, R.get_launch()['block']
    counts = counts_of(1, E - 1, E, E + 1, 2 * E + 1, B * E - 1, B * E, B * E + 1,
                       2 * B * E + E + 1, 4099)
    ops = multi_operands(t, max(counts), k, 'A1')
    exp = multi_oracle(oracle, t, max(counts), ops[0], ops[1:])
    for phase in sorted({0, t.ext % 16, (16 - t.ext) % 16}):
        for n in counts:
            check_multi(R, t, n, ops[0], ops[1:], phase, [phase] * k, exp, (n, phase))


@pytest.mark.parametrize('k', [2, 16])
@pytest.mark.parametrize('dtname,opname', EDGE_TYPES, ids=EDGE_IDS)
def test_multi_mixed_phases(R, H, oracle, dtname, opname, k):
    """A2, k_elem_multi: one input (the first, a middle one, the last) or the
    inout alone an element off the others' phase, and for multi-byte units
    one operand half an element off the element grid.  (A 16-byte unit keeps
    its phase an element on: there only the half element leaves the packet
    kernel.)"""
    t = ty(R, H, dtname, opname)
    counts = counts_of(1, 2 * t.E + 1, 4099)
    ops = multi_operands(t, max(counts), k, 'A2')
    exp = multi_oracle(oracle, t, max(counts), ops[0], ops[1:])
    places = []
    for q in sorted({0, k // 2, k - 1}):
        places.append((0, [t.ext if j == q else 0 for j in range(k)]))
    places.append((t.ext, [0] * k))
    if t.ext >= 2:
        half = t.ext // 2
        places.append((half, [0] * k))
        places.append((0, [half if j == k // 2 else 0 for j in range(k)]))
    for io_off, in_offs in places:
        for n in counts:
            check_multi(R, t, n, ops[0], ops[1:], io_off, in_offs, exp, (n, io_off, in_offs))


@pytest.mark.parametrize('dtname', ['MPI_FLOAT', 'MPIX_C_FLOAT16'])
def test_multi_block_sizes_and_looping_grid(R, H, oracle, dtname):
    """A3: launch_multi honours the block and the grid limit: the grid-stride
    loop goes round several times, and at 1024 threads the unused LDS that caps
    the waves per SIMD (kMultiLds per wave) passes 64 KiB and is dropped"""
    t = ty(R, H, dtname, 'MPI_SUM')
    k, n = 3, 65536 + 5
    ops = multi_operands(t, n, k, 'A3')
    exp = multi_oracle(oracle, t, n, ops[0], ops[1:])
    before = R.get_launch()
    try:
        for block, max_grid in ((64, 2), (512, 3), (1024, 1)):
            assert R.set_launch(block, max_grid) == 0
            now = R.get_launch()
            assert (now['block'], now['max_grid']) == (block, max_grid)
            for phase in (0, 16 - t.ext):       # 16 - ext: a one-element head
                check_multi(R, t, n, ops[0], ops[1:], phase, [phase] * k, exp,
                            (block, max_grid, phase))
    finally:
        assert R.set_launch(before['block'], before['max_grid']) == 0
    assert R.get_launch() == before


def _special_f16(rng, n):
    """halves with NaN (two payloads), +-0 and Inf mixed in"""
    x = rng.uniform(-1, 1, n).astype(np.float16).view(np.uint16)
    pick = rng.integers(0, 8, n)
    for p, bits in ((0, 0x0000), (1, 0x8000), (2, 0x7e01), (3, 0xfe55), (4, 0x7c00)):
        x[pick == p] = bits
    return x.view(np.uint8)


@pytest.mark.parametrize('dtname,opname', [('MPI_DOUBLE', 'MPI_MAX'), ('MPI_DOUBLE', 'MPI_MIN'),
                                           ('MPIX_C_FLOAT16', 'MPI_MAX')])
def test_multi_operand_roles(R, H, oracle, dtname, opname):
    """A4: MAX / MIN choose by operand role where the values compare equal or
    unordered (NaN payloads, +-0), so a swapped inout / in shows in the bits;
    both kernels"""
    t = ty(R, H, dtname, opname)
    k, n = 3, 4099
    rng = np.random.default_rng(seed(dtname, opname, 'A4'))
    gen = (lambda: _special_f64(rng, n).view(np.uint8)) if dtname == 'MPI_DOUBLE' else \
        (lambda: _special_f16(rng, n))
    ops = [gen() for _ in range(k + 1)]
    exp = multi_oracle(oracle, t, n, ops[0], ops[1:])
    for in_offs in ([0, 0, 0], [0, t.ext, 0]):
        got = check_multi(R, t, n, ops[0], ops[1:], 0, in_offs, exp, in_offs)
        assert np.array_equal(got, exp)     # MAX / MIN: payloads and signs pinned, too


@pytest.mark.parametrize('k', [3, 16])
@pytest.mark.parametrize('dtname', ['MPI_COMPLEX4', 'MPI_C_FLOAT_COMPLEX', 'MPI_C_DOUBLE_COMPLEX'])
def test_multi_complex_product_nan_bits(R, H, oracle, dtname, k):
    """each part of a complex product adds two terms; where both are NaN the
    sum returns one of them, and the packet and element kernels of the fold
    once chose differently from the single call's (a NaN's sign differed on
    MPI_C_FLOAT_COMPLEX at k = 3 and on MPI_COMPLEX4 at k = 16): operands
    with 1 % of NaN and Inf parts, every product folding earlier NaNs in"""
    t = ty(R, H, dtname, 'MPI_PROD')
    n = 4099
    ops = multi_operands(t, n, k, 'probe')
    exp = multi_oracle(oracle, t, n, ops[0], ops[1:])
    for in_offs in ([0] * k, [t.ext] + [0] * (k - 1), [t.ext // 2] + [0] * (k - 1)):
        check_multi(R, t, n, ops[0], ops[1:], 0, in_offs, exp, in_offs)


@pytest.mark.parametrize('dtname,opname,zero_im', [('MPI_LONG_DOUBLE_INT', 'MPI_MAXLOC', False),
                                                   ('MPI_COMPLEX32', 'MPI_PROD', True)])
def test_multi_wide_units(R, H, oracle, dtname, opname, zero_im):
    """32-byte units always run k_elem_multi"""
    t = ty(R, H, dtname, opname)
    k = 3
    rng = np.random.default_rng(seed(dtname, 'A5'))
    for n in (1, 65, 1027):
        ops = [x.reshape(-1) for _ in range(2) for x in _soft_operands(H, rng, dtname, n, zero_im)]
        exp = multi_oracle(oracle, t, n, ops[0], ops[1:])
        for io_off, in_offs in ((0, [0, 0, 0]), (16, [0, 16, 0])):
            check_multi(R, t, n, ops[0], ops[1:], io_off, in_offs, exp, (n, io_off))


# ------------------------------------------------------------- tree fold
def tree_oracle(oracle, t, n, vals, pres):
    nb = n * t.ext
    v = [x[:nb] for x in vals]
    for kind, s, r in M.tree_steps(len(v), pres):
        if kind == 'op':
            acc = v[s].copy()
            assert oracle.reduce_local(v[r].copy(), acc, n, t.dt, t.op) == 0
            v[s] = acc
        else:
            v[s] = v[r]
    return v[0]


def check_tree(R, oracle, t, n, vals, S, pres, out_off, in_place, ctx):
    """one tree fold of the first n elements of the slots `vals`, already on
    the device as S (all k of them; the absent ones are not passed), into a
    separate output at byte offset out_off or in place over slot `in_place`"""
    k, nb = len(vals), n * t.ext
    ctx = (bin(pres), n, in_place) + tuple(ctx)
    present = [q for q in range(k) if (pres >> q) & 1]
    steps = M.tree_steps(k, pres)
    exp = tree_oracle(oracle, t, n, vals, pres)
    slots = list(S)
    if in_place is None:
        out = place(np.full(nb, CANARY, np.uint8), out_off)
    else:
        out = slots[in_place] = place(vals[in_place][:nb], S[in_place].off)
    # the single calls work on copies of the slots they write
    written = {s for _, s, _ in steps}
    W = {q: device_copy(S[q]) if q in written else S[q] for q in present}
    torch.cuda.synchronize()
    assert R.reduce_local_tree_async([slots[q].v if q in present else None for q in range(k)],
                                     out.v, n, t.dt, t.op) == 0, ctx
    for kind, s, r in steps:
        if kind == 'op':
            assert R.reduce_local_async(W[r].v, W[s].v, n, t.dt, t.op) == 0, ctx
        else:
            W[s] = place(np.zeros(nb, np.uint8), S[s].off)
            W[s].v.copy_(W[r].v)
    got, ref = read(out, ctx), read(W[0], ctx)
    for q in present:
        if q != in_place:
            assert np.array_equal(read(slots[q], ctx), vals[q][:nb]), ('input changed', q, ctx)
    assert np.array_equal(got, ref), ('differs from the single calls', ctx)
    assert oracle_mismatches(t, got, exp) == 0, ('oracle', ctx)
    return got


def tree_tile(k):
    """packets per block of the packet form at k slots (launch_tree)"""
    return 128 if k <= 4 else 64


# MAXLOC on integer pairs is commutative (a tie takes the smaller loc, there is
# no NaN and no padding), so MPI_2INT shows a wrong slot or mask but not a
# swapped role; MPI_FLOAT_INT, the same 8-byte unit with NaN values (the inout
# is kept), shows that too
MASK_TYPES = [('MPI_FLOAT', 'MPI_SUM'), ('MPI_DOUBLE', 'MPI_MIN'), ('MPI_2INT', 'MPI_MAXLOC'),
              ('MPI_FLOAT_INT', 'MPI_MAXLOC'), ('MPI_INT8_T', 'MPI_MAX'),
              ('MPI_DOUBLE_INT', 'MPI_MINLOC'), ('MPI_FLOAT', 'MPI_REPLACE'),
              ('MPI_FLOAT', 'MPI_NO_OP')]


def tree_operands(t, n, k, *salt):
    rng = np.random.default_rng(seed(t.dtname, t.opname, k, *salt))

    def one():
        if t.dtname == 'MPI_DOUBLE':
            return _special_f64(rng, n).view(np.uint8)
        if t.dtname == 'MPI_2INT':      # few values: ties are frequent, the locs decide
            return np.stack([rng.integers(0, 3, n), rng.integers(0, 50, n)], 1) \
                .astype('<i4').view(np.uint8).reshape(-1)
        return make_operand(rng, t.kind, t.size, n, t.dtname)
    return [one() for _ in range(k)]


def phase_step(t):
    """the smallest whole-element step that leaves the 16-byte phase; a
    16-byte unit has none, so half an element"""
    return t.ext if t.ext < 16 else 8


@pytest.mark.parametrize('path', ['one_phase', 'slot_off', 'out_off'])
@pytest.mark.parametrize('k', [2, 4, 8, 16])
@pytest.mark.parametrize('dtname,opname', MASK_TYPES, ids=['%s-%s' % m for m in MASK_TYPES])
def test_tree_presence_masks(R, H, oracle, dtname, opname, k, path):
    """B1: both-present, right-only and left-only at every node of every
    level, and the presence propagated upwards: every mask up to k = 8,
    fold_model.masks_for(16) at 16.  A full tile, a partial one, a head and a
    tail behind a one-element head; on one phase (the packet form of this k),
    with one present slot or only the output off it (k_elem_tree, units of at
    most 16 bytes)"""
    t = ty(R, H, dtname, opname)
    n = 2 * tree_tile(k) * t.E + t.E + 1
    base, step = t.ext, phase_step(t)
    vals = tree_operands(t, n, k, 'B1')
    S = [place(x, base) for x in vals]
    S_off = [place(x, base + step) for x in vals] if path == 'slot_off' else None
    for i, pres in enumerate(M.masks_for(k)):
        slots, out_off = S, base
        if path == 'slot_off':
            present = [q for q in range(k) if (pres >> q) & 1]
            q = present[i % len(present)]
            slots = S[:q] + [S_off[q]] + S[q + 1:]
        elif path == 'out_off':
            out_off = base + step
        check_tree(R, oracle, t, n, vals, slots, pres, out_off, None, (path,))


SPARSE = {2: 0b01, 4: 0b1001, 8: 0b10100101, 16: 0b1000010000101001}


@pytest.mark.parametrize('k', [2, 4, 8, 16])
@pytest.mark.parametrize('dtname', ['MPI_COMPLEX4', 'MPI_C_FLOAT_COMPLEX', 'MPI_C_DOUBLE_COMPLEX'])
def test_tree_complex_product_nan_bits(R, H, oracle, dtname, k):
    """test_multi_complex_product_nan_bits for the four packet forms of the
    tree and for k_elem_tree"""
    t = ty(R, H, dtname, 'MPI_PROD')
    n = 4099
    vals = tree_operands(t, n, k, 'nan')
    S = [place(x, 0) for x in vals]
    last_off = [place(vals[k - 1], t.ext // 2)]
    for pres in ((1 << k) - 1, SPARSE[k] | (1 << (k - 1))):
        check_tree(R, oracle, t, n, vals, S, pres, 0, None, ('packet',))
        check_tree(R, oracle, t, n, vals, S[:k - 1] + last_off, pres, 0, None, ('element',))


@pytest.mark.parametrize('k', [2, 4, 8, 16])
@pytest.mark.parametrize('dtname,opname', [('MPI_FLOAT', 'MPI_SUM'), ('MPI_INT16_T', 'MPI_BXOR'),
                                           ('MPI_INTEGER16', 'MPI_SUM')])
def test_tree_count_edges(R, H, oracle, dtname, opname, k):
    """B2: each packet form below its head, without a packet, at one packet,
    at one tile and a packet either side (the i + u*nt < npk guards of the
    two-packet forms) and over two tiles; separate output and in place over
    the first, a middle and the last present slot; on the 16-byte grid and
    behind a one-element head"""
    t = ty(R, H, dtname, opname)
    E, P = t.E, tree_tile(k)
    counts = counts_of(1, E - 1, E, E + 1, P * E - 1, P * E, P * E + 1, 2 * P * E + E + 1)
    vals = tree_operands(t, max(counts), k, 'B2')
    for off in sorted({0, t.ext % 16}):
        S = [place(x, off) for x in vals]
        for pres in ((1 << k) - 1, SPARSE[k]):
            present = [q for q in range(k) if (pres >> q) & 1]
            outs = [None] + sorted({present[0], present[len(present) // 2], present[-1]})
            for n in counts:
                Sn = S if n == max(counts) else [place(x[:n * t.ext], off) for x in vals]
                for in_place in outs:
                    check_tree(R, oracle, t, n, vals, Sn, pres, off, in_place, (off,))


@pytest.mark.parametrize('k', [2, 4, 8])
@pytest.mark.parametrize('dtname,opname,zero_im', [('MPI_LONG_DOUBLE_INT', 'MPI_MAXLOC', False),
                                                   ('MPI_COMPLEX32', 'MPI_PROD', False),
                                                   ('MPI_COMPLEX32', 'MPI_PROD', True)],
                         ids=['LONG_DOUBLE_INT-MAXLOC', 'COMPLEX32-PROD', 'COMPLEX32-PROD-real'])
def test_tree_wide_units(R, H, oracle, dtname, opname, zero_im, k):
    """B3: 32-byte units run k_elem_tree's tree_fold_rec<0, 16> branch at every
    k above 2: x87 specials under MAXLOC, the binary128 complex product on its
    fast path and (zero imaginary parts) on the general one.  At k = 2 with
    both slots present and everything on the 16-byte grid they run k_contig32
    (the product its two launches; over slot 1 k_elem_tree, launch_tree).
    Output: separate, over slot 0, over slot 1 and over the last present slot"""
    t = ty(R, H, dtname, opname)
    rng = np.random.default_rng(seed(dtname, zero_im, k, 'B3'))
    masks = [(1 << k) - 1, 1, SPARSE[k], M.odd_upper_absent(k) & ~2]
    for n in (1, 65, 1027):
        vals = [x.reshape(-1) for _ in range(k // 2)
                for x in _soft_operands(H, rng, dtname, n, zero_im)]
        for offs, out_off in (([0] * k, 0), ([16 * (q % 2) for q in range(k)], 16)):
            S = [place(x, o) for x, o in zip(vals, offs)]
            for pres in dict.fromkeys(masks):
                last = pres.bit_length() - 1
                outs = [None, 0] + sorted({q for q in (1, last) if q and (pres >> q) & 1})
                for in_place in outs:
                    check_tree(R, oracle, t, n, vals, S, pres, out_off, in_place, (offs[1],))
