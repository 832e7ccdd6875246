"""Typed accumulate and get-accumulate (MPIX_[Get_]accumulate_local_typed*: a
committed plan on the origin, the result and the target side) on the GPU.

Every case is checked three ways:
  (a) against the oracle: numpy gather of the origin by its runs, the oracle's
      iov apply on a host copy of the target, numpy scatter of the old
      target's type map into the result layout -- result and target over their
      whole buffers;
  (b) bit for bit over the WHOLE buffers (gaps, padding and guard bytes
      included) against the three-step composition of the existing entries on
      device copies: gather the origin (MPIX_Get_accumulate_local_plan, NO_OP),
      the packed-origin plan entry, scatter the packed result
      (MPIX_Reduce_local_plan, REPLACE); a packed side needs no step of its own,
      so with both packed the twin is MPIX_Get_accumulate_local_plan /
      MPIX_Reduce_local_plan itself;
  (c) the origin unchanged, the guard bytes of all three buffers intact.
"""
import threading

import numpy as np
import pytest
import torch

from tests.test_getacc_gpu import CANARY, Placed, _soft_operands, field_mask
from tests.test_getacc_iov_gpu import MANY, gather, layout, operands, run_mask
from tests.test_gpu_parity import SWEEP, compare, make_operand
from tests.test_iovec import PAIRS, pair_iov, random_pairs
from tests.test_plan_gpu import SWEEP_LENS, TILE_LENS

pytestmark = pytest.mark.gpu


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


class Side:
    """one operand of a typed call: its bytes on the host, its layout as
    element runs (offs, cnts) from byte `base` of the buffer, its plan (None: a
    packed operand), and the bytes placed on the device `shift` bytes off a
    256-byte boundary"""

    def __init__(self, R, dt, data, total, offs=None, cnts=None, base=0, shift=0, plan=None,
                 iovec=None, device='cuda'):
        self.host = np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy()
        self.base, self.shift, self.device = base, shift, device
        self.own = False
        if offs is None:
            self.offs, self.cnts, self.plan = [0], [total], None
            assert plan is None
        else:
            self.offs, self.cnts = list(offs), list(cnts)
            assert sum(cnts) == total
            self.plan = plan
            if plan is None:
                self.own = True
                self.plan = R.IovPlan.from_iovec(iovec[0], iovec[1], dt) if iovec else \
                    R.IovPlan.from_iov(self.offs, self.cnts, dt)
        self.P = Placed(self.host, shift, device=device)

    @property
    def v(self):
        return self.P.v[self.base:]

    def twin(self):
        t = object.__new__(Side)
        t.__dict__.update(self.__dict__)
        t.own = False
        t.P = Placed(self.host, self.shift, device=self.device)
        return t

    def close(self):
        if self.own:
            self.plan.close()


def typed_call(R, op, O, Z, T, fetch=True, sync=False, stream=None):
    o, oplan = (None, None) if O is None else (O.v, O.plan)
    if fetch:
        return R.get_accumulate_local_typed(o, oplan, Z.v, Z.plan, T.v, T.plan, op, sync=sync,
                                            stream=stream)
    return R.accumulate_local_typed(o, oplan, T.v, T.plan, op, sync=sync, stream=stream)


def composition(R, H, op, O, Z, T, ext, total, fetch=True, stream=None):
    """the same call as three steps of the existing entries, on its own buffers"""
    nb = total * ext
    po = None
    if O is not None:
        po = O.v
        if O.plan is not None:
            po = torch.full((nb,), 0x11, dtype=torch.uint8, device=O.device)
            assert R.get_accumulate_local_plan(None, po, O.v, O.plan, H.MPI_NO_OP,
                                               stream=stream) == 0
    if not fetch:
        if op != H.MPI_NO_OP:
            assert R.reduce_local_plan(po, T.v, T.plan, op, stream=stream) == 0
        return
    pr = Z.v
    if Z.plan is not None:
        pr = torch.full((nb,), 0x22, dtype=torch.uint8, device=Z.device)
    assert R.get_accumulate_local_plan(po, pr, T.v, T.plan, op, stream=stream) == 0
    if Z.plan is not None:
        assert R.reduce_local_plan(pr, Z.v, Z.plan, H.MPI_REPLACE, stream=stream) == 0


def element_bytes(side, ext, mask):
    """byte indices, per packed element, of the type map in the side's buffer"""
    pos = np.concatenate([side.base + o + ext * np.arange(c, dtype=np.int64)
                          for o, c in zip(side.offs, side.cnts) if c] or
                         [np.zeros(0, np.int64)])
    return pos[:, None] + np.nonzero(mask)[0][None, :]


def expectation(H, oracle, dt, op, O, Z, T, ext, total, fetch):
    """(a): the oracle's target and the scattered result, as whole buffers"""
    before = gather(T.host, T.base, T.offs, T.cnts, ext)
    packed = np.zeros(max(total * ext, 1), np.uint8) if O is None else \
        gather(O.host, O.base, O.offs, O.cnts, ext).copy()
    exp_t = T.host.copy()
    assert oracle.reduce_local_iov(packed, exp_t[T.base:], T.offs, T.cnts, dt, op) == 0
    exp_z = None
    if fetch:
        exp_z = Z.host.copy()
        m = field_mask(H, dt, ext)
        exp_z[element_bytes(Z, ext, m)] = before.reshape(total, ext)[:, m]
    return exp_t, exp_z


def check(R, H, oracle, dt, op, O, Z, T, O2, Z2, T2, fetch=True, parity=None):
    """after synchronising: (a), (b), (c); returns the target's bytes"""
    ext = R.datatype_extent(dt)
    total = sum(T.cnts)
    exp_t, exp_z = expectation(H, oracle, dt, op, O, Z, T, ext, total, fetch)
    got = T.P.bytes()
    if parity:
        kind, size, opname = parity
        assert compare(gather(got, T.base, T.offs, T.cnts, ext),
                       gather(exp_t, T.base, T.offs, T.cnts, ext), kind, size, opname,
                       ext) == 0, '(a) target against the oracle'
        gaps = ~run_mask(len(got), T.base, T.offs, T.cnts, ext)
        assert np.array_equal(got[gaps], T.host[gaps]), '(a) a gap byte of the target changed'
    else:
        assert np.array_equal(got, exp_t), '(a) target against the oracle'
    assert np.array_equal(got, T2.P.bytes()), '(b) target differs from the composition'
    if fetch:
        z = Z.P.bytes()
        assert np.array_equal(z, exp_z), '(a) result'
        assert np.array_equal(z, Z2.P.bytes()), '(b) result differs from the composition'
        assert Z.P.guards_intact() and Z2.P.guards_intact(), '(c) result guards'
    if O is not None:
        assert np.array_equal(O.P.bytes(), O.host), '(c) origin changed'
        assert O.P.guards_intact(), '(c) origin guards'
    assert T.P.guards_intact() and T2.P.guards_intact(), '(c) target guards'
    return got


def run_case(R, H, oracle, dt, op, O, Z, T, fetch=True, parity=None, sync=False, prepare=True):
    """one typed call and its composition twin; closes the sides' own plans"""
    ext = R.datatype_extent(dt)
    total = sum(T.cnts)
    try:
        if prepare:
            assert T.plan.prepare() == 0
            for s in (O, Z):
                if s is not None and s.plan is not None:
                    assert s.plan.prepare_packed() == 0
                    assert s.plan.prepare_packed() == 0     # idempotent
        O2, Z2, T2 = (None if s is None else s.twin() for s in (O, Z, T))
        torch.cuda.synchronize()
        assert typed_call(R, op, O, Z, T, fetch, sync) == 0
        composition(R, H, op, O2, Z2, T2, ext, total, fetch)
        torch.cuda.synchronize()
        return check(R, H, oracle, dt, op, O, Z, T, O2, Z2, T2, fetch, parity)
    finally:
        torch.cuda.synchronize()
        for s in (O, Z, T):
            if s is not None:
                s.close()


def derived(R, rng, dt, ext, lens, data_of, total, shift=0, gap=(1, 6)):
    """a side of `lens` runs with gaps from the `layout` helper; data_of(span)
    makes its buffer's elements"""
    offs, span = layout(rng, lens, ext, gap)
    return Side(R, dt, data_of(span), total, offs, lens, shift=shift)


def canary(n, ext):
    return np.full(n * ext, CANARY, np.uint8)


def fp64_sides(R, H, rng, tl, ol, zl, shifts=(0, 0, 0)):
    """fp64 origin / result / target of runs ol / zl / tl (None: packed)"""
    n = sum(tl)
    mk = lambda span: make_operand(rng, 'fp', 8, span, 'MPI_DOUBLE')      # noqa: E731
    T = derived(R, rng, H.MPI_DOUBLE, 8, tl, mk, n, shifts[2])
    O = Side(R, H.MPI_DOUBLE, mk(n), n, shift=shifts[0]) if ol is None else \
        derived(R, rng, H.MPI_DOUBLE, 8, ol, mk, n, shifts[0])
    Z = Side(R, H.MPI_DOUBLE, canary(n, 8), n, shift=shifts[1]) if zl is None else \
        derived(R, rng, H.MPI_DOUBLE, 8, zl, lambda span: canary(span, 8), n, shifts[1])
    return O, Z, T


# 1 ------------------------------------------------------------ misaligned cuts
O_LENS, Z_LENS = [256, 1, 560], TILE_LENS[::-1]


def test_misaligned_cuts(R, H, oracle):
    """817 fp64 elements cut at 255 / 256 / 257 / 512 / 812 in the target, at
    256 / 257 in the origin and at 5 / 305 / 560 / 561 / 562 in the result"""
    assert sum(TILE_LENS) == sum(O_LENS) == sum(Z_LENS) == 817
    rng = np.random.default_rng(0x5EED1210)
    for op in (H.MPI_SUM, H.MPI_REPLACE, H.MPI_NO_OP):
        for fetch in (True, False):
            O, Z, T = fp64_sides(R, H, rng, TILE_LENS, O_LENS, Z_LENS, (8, 16, 0))
            run_case(R, H, oracle, H.MPI_DOUBLE, op, O, Z, T, fetch, ('fp', 8, 'MPI_SUM'))
    O, Z, T = fp64_sides(R, H, rng, TILE_LENS, O_LENS, Z_LENS)
    run_case(R, H, oracle, H.MPI_DOUBLE, H.MPI_PROD, O, Z, T, True, ('fp', 8, 'MPI_PROD'),
             prepare=False)


def test_misaligned_cuts_capped_grid(R, H, oracle):
    """max_grid = 2 on three of it in a row: each block walks every other tile"""
    rng = np.random.default_rng(0x5EED1211)
    before = R.get_launch()
    assert R.set_launch(before['block'], 2) == 0
    try:
        assert 3 * 817 > 2 * 1024
        for op in (H.MPI_SUM, H.MPI_REPLACE, H.MPI_NO_OP):
            for fetch in (True, False):
                O, Z, T = fp64_sides(R, H, rng, TILE_LENS * 3, O_LENS * 3, Z_LENS * 3)
                run_case(R, H, oracle, H.MPI_DOUBLE, op, O, Z, T, fetch, ('fp', 8, 'MPI_SUM'))
    finally:
        assert R.set_launch(before['block'], before['max_grid']) == 0
    assert R.get_launch() == before


# 2 ------------------------------------------------------------------------ roles
def role_runs(kind, n, cut):
    """(lens, first offset in elements) of a side: 'one' a single run at a
    non-zero offset, 'multi' runs cut at `cut`"""
    if kind == 'one':
        return [n], (3, 4)
    return [x for x in (cut, 1, n - cut - 1) if x > 0] if n > 2 else [1] * n, (1, 6)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('dtname,size', [('MPI_FLOAT', 4), ('MPI_DOUBLE', 8)])
def test_roles(R, H, oracle, dtname, size, n):
    """origin and result each NULL plan / one run at a non-zero offset /
    multi-run, the target one run / multi-run.  With both plans NULL the twin
    of (b) is MPIX_Get_accumulate_local_plan / MPIX_Reduce_local_plan itself."""
    dt = getattr(H, dtname)
    rng = np.random.default_rng(0x5EED1220 + 16 * n + size)
    mk = lambda span: make_operand(rng, 'fp', size, span, dtname)       # noqa: E731
    kinds = ('null', 'one', 'multi') if n > 1 else ('null', 'one')
    done = 0
    for tk in kinds[1:]:
        for ok in kinds:
            for zk in kinds:
                sides = []
                for k, cut, data in ((ok, n // 3, mk), (zk, 1, lambda s: canary(s, size)),
                                     (tk, n // 2, mk)):
                    if k == 'null':
                        sides.append(Side(R, dt, data(n), n, shift=size))
                    else:
                        lens, gap = role_runs(k, n, cut)
                        sides.append(derived(R, rng, dt, size, lens, data, n, gap=gap))
                        assert sides[-1].plan.info()['runs'] == len(lens)
                        assert sides[-1].plan.locate(0) != 0
                O, Z, T = sides
                for fetch in ((False, True) if zk == 'null' else (True,)):   # twins first
                    o, z, t = (O, Z, T) if fetch else (O.twin(), None, T.twin())
                    run_case(R, H, oracle, dt, H.MPI_SUM, o, z, t, fetch, ('fp', size, 'MPI_SUM'),
                             prepare=bool(done & 1))
                    done += 1
    assert done == (24 if n > 1 else 6)


# 3 ------------------------------------------------------------ order and residues
def two_residues(R, rng, dt, lens, data_of):
    """test_plan_gpu's shape: slots shuffled against the packed order, offsets
    below the buffer pointer, shifted by 0, 4 and -12 bytes in turn"""
    slots, span = layout(rng, lens, 8, gap=(3, 6))
    order = rng.permutation(len(lens))
    base = (span // 2) * 8
    offs = [slots[j] + 8 + (0, 4, -12)[i % 3] - base for i, j in enumerate(order)]
    cnts = [lens[j] for j in order]
    assert min(offs) < 0 < max(offs) and {o % 8 for o, c in zip(offs, cnts) if c} == {0, 4}
    s = Side(R, dt, data_of(span + 2), sum(lens), offs, cnts, base=base)
    assert s.plan.info()['groups'] == 2 and s.plan.info()['lo_byte'] < 0
    return s


def cuts_of(rng, total, k):
    """k run lengths (some zero) adding up to `total`"""
    c = np.sort(rng.integers(0, total + 1, k - 1))
    return [int(x) for x in np.diff(np.concatenate([[0], c, [total]]))]


def test_two_residue_groups_shuffled_order_negative_offsets(R, H, oracle):
    rng = np.random.default_rng(0x5EED1230)
    mk = lambda span: make_operand(rng, 'fp', 8, span, 'MPI_DOUBLE')      # noqa: E731
    total = 1400
    for op, fetch in ((H.MPI_SUM, True), (H.MPI_SUM, False), (H.MPI_REPLACE, True)):
        T = two_residues(R, rng, H.MPI_DOUBLE, cuts_of(rng, total, 60), mk)
        O = two_residues(R, rng, H.MPI_DOUBLE, cuts_of(rng, total, 45), mk)
        Z = two_residues(R, rng, H.MPI_DOUBLE, cuts_of(rng, total, 75), lambda s: canary(s, 8))
        run_case(R, H, oracle, H.MPI_DOUBLE, op, O, Z, T, fetch, ('fp', 8, 'MPI_SUM'))


# 4 ------------------------------------------------------- one handle, three roles
def test_one_handle_in_all_three_roles(R, H, oracle):
    rng = np.random.default_rng(0x5EED1240)
    offs, span = layout(rng, TILE_LENS, 8)
    mk = lambda: make_operand(rng, 'fp', 8, span, 'MPI_DOUBLE')         # noqa: E731
    with R.IovPlan.from_iov(offs, TILE_LENS, H.MPI_DOUBLE) as p:
        for op, fetch in ((H.MPI_SUM, True), (H.MPI_MAX, True), (H.MPI_SUM, False)):
            O = Side(R, H.MPI_DOUBLE, mk(), 817, offs, TILE_LENS, plan=p)
            Z = Side(R, H.MPI_DOUBLE, canary(span, 8), 817, offs, TILE_LENS, plan=p, shift=8)
            T = Side(R, H.MPI_DOUBLE, mk(), 817, offs, TILE_LENS, plan=p)
            run_case(R, H, oracle, H.MPI_DOUBLE, op, O, Z, T, fetch, ('fp', 8, 'MPI_SUM'))


# 5 --------------------------------------------------------------------- type sweep
SWEEP_O, SWEEP_Z = [256, 1, 343], SWEEP_LENS[::-1]


def sweep_sides(R, H, rng, dtname, kind, size, zero_im=None):
    dt = getattr(H, dtname)
    ext = R.datatype_extent(dt)
    n = sum(SWEEP_LENS)
    assert n == sum(SWEEP_O) == 600
    toffs, tspan = layout(rng, SWEEP_LENS, ext)
    ooffs, ospan = layout(rng, SWEEP_O, ext)
    if zero_im is None:
        tgt, org = operands(H, rng, dtname, kind, size, tspan, ospan)
    else:
        tgt, org = _soft_operands(H, rng, dtname, max(tspan, ospan), zero_im)
        tgt, org = tgt.reshape(-1)[:tspan * 32], org.reshape(-1)[:ospan * 32]
    T = Side(R, dt, tgt, n, toffs, SWEEP_LENS)
    O = Side(R, dt, org, n, ooffs, SWEEP_O, shift=ext)
    Z = derived(R, rng, dt, ext, SWEEP_Z, lambda s: canary(s, ext), n)
    assert [s.plan.info()['runs'] for s in (O, Z, T)] == [3, 5, 5]
    return dt, O, Z, T


@pytest.mark.parametrize('dtname,opname,kind,size', SWEEP,
                         ids=['%s-%s' % (s[0], s[1]) for s in SWEEP])
def test_every_pair(R, H, oracle, dtname, opname, kind, size):
    """all three sides multi-run, at test_plan_gpu.py::test_every_pair's count"""
    op = getattr(H, opname)
    rng = np.random.default_rng((0x5EED1250 * 31 + getattr(H, dtname) * 7 + op) & 0xffffffff)
    dt, O, Z, T = sweep_sides(R, H, rng, dtname, kind, size)
    run_case(R, H, oracle, dt, op, O, Z, T, True, (kind, size, opname))


@pytest.mark.parametrize('dtname', ['MPI_COMPLEX32', 'MPI_C_LONG_DOUBLE_COMPLEX'])
def test_wide_complex_products(R, H, oracle, dtname):
    rng = np.random.default_rng(0x5EED1251 + (getattr(H, dtname) & 0xff))
    for zero_im in (False, True):
        for fetch in (True, False):
            dt, O, Z, T = sweep_sides(R, H, rng, dtname, 'soft', None, zero_im)
            run_case(R, H, oracle, dt, H.MPI_PROD, O, Z, T, fetch)


# 6 ------------------------------------------- padded pairs through iovec plans
def raw_iov(R, H, dt, pos):
    """{value, int} segments of the elements at `pos`, unmerged"""
    if dt in PAIRS:
        return pair_iov(dt, pos, False)
    assert dt == H.MPI_LONG_DOUBLE_INT and R.datatype_size(dt) == 20
    offs, lens = [], []
    for p in pos:
        offs += [32 * p, 32 * p + 16]
        lens += [16, 4]
    return offs, lens


def pair_side(R, H, rng, dt, ext, n, span, data, shift=0):
    pos = sorted(rng.choice(span, n, replace=False).tolist())
    return Side(R, dt, data, n, [p * ext for p in pos], [1] * n, shift=shift,
                iovec=raw_iov(R, H, dt, pos))


@pytest.mark.parametrize('opname', ['MPI_MAXLOC', 'MPI_MINLOC', 'MPI_REPLACE', 'MPI_NO_OP'])
@pytest.mark.parametrize('dtname', ['MPI_DOUBLE_INT', 'MPI_SHORT_INT', 'MPI_LONG_DOUBLE_INT'])
def test_padded_pairs_through_iovec_plans(R, H, oracle, dtname, opname):
    """the type map only: the result's and the origin's padding bytes stay
    ((a) compares the whole result buffer, (c) the whole origin)"""
    dt, op = getattr(H, dtname), getattr(H, opname)
    ext = R.datatype_extent(dt)
    rng = np.random.default_rng(0x5EED1260 + (dt & 0xff) * 8 + (op & 0xf))
    n, span = 300, 420
    assert not field_mask(H, dt, ext).all()
    if dt in PAIRS:
        tgt, org = random_pairs(rng, dt, span), random_pairs(rng, dt, span)
    else:
        tgt, org = operands(H, rng, dtname, 'soft', None, span, span)
    for fetch in (True, False):
        T = pair_side(R, H, rng, dt, ext, n, span, tgt)
        O = pair_side(R, H, rng, dt, ext, n, span, org, shift=ext)
        Z = pair_side(R, H, rng, dt, ext, n, span, rng.integers(0, 256, span * ext, dtype=np.uint8))
        assert T.plan.info()['runs'] > 1 and O.plan.info()['elements'] == n
        run_case(R, H, oracle, dt, op, O, Z, T, fetch)


# 7 ------------------------------------------------------------- NO_OP and REPLACE
@pytest.mark.parametrize('dtname,kind,size', MANY, ids=[m[0] for m in MANY])
def test_no_op_and_replace(R, H, oracle, dtname, kind, size):
    """MPI_Get / the swap / MPI_Put / nothing over 330 runs a side"""
    dt = getattr(H, dtname)
    ext = R.datatype_extent(dt)
    rng = np.random.default_rng(0x5EED1270 + len(dtname))
    mk = lambda span: make_operand(rng, kind, size, span, dtname)       # noqa: E731
    m = field_mask(H, dt, ext)

    def sides():
        total = 990
        T = derived(R, rng, dt, ext, cuts_of(rng, total, 330), mk, total, gap=(1, 4))
        O = derived(R, rng, dt, ext, cuts_of(rng, total, 200), mk, total, gap=(1, 4), shift=ext)
        Z = derived(R, rng, dt, ext, cuts_of(rng, total, 280), lambda s: canary(s, ext), total,
                    gap=(1, 4))
        return O, Z, T
    # the fetch form's MPI_NO_OP: neither origin nor origin_plan is looked at
    O, Z, T = sides()
    O.close()
    T.plan.prepare(), Z.plan.prepare_packed()
    torch.cuda.synchronize()
    junk = 0xdead0
    assert R.lib().MPIX_Get_accumulate_local_typed_async(
        None, junk, Z.v.data_ptr(), Z.plan.handle, T.v.data_ptr(), T.plan.handle,
        H.as_c_int(H.MPI_NO_OP), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(T.P.bytes(), T.host)
    got = gather(Z.P.bytes(), 0, Z.offs, Z.cnts, ext).reshape(-1, ext)
    assert np.array_equal(got[:, m], gather(T.host, 0, T.offs, T.cnts, ext).reshape(-1, ext)[:, m])
    Z.close(), T.close()
    O, Z, T = sides()
    O.close()
    assert np.array_equal(run_case(R, H, oracle, dt, H.MPI_NO_OP, None, Z, T), T.host)
    # the accumulate form's MPI_NO_OP touches nothing
    O, Z, T = sides()
    Z.close()
    assert np.array_equal(run_case(R, H, oracle, dt, H.MPI_NO_OP, O, None, T, fetch=False), T.host)
    # MPI_REPLACE: the swap and MPI_Put
    for fetch in (True, False):
        O, Z, T = sides()
        got = run_case(R, H, oracle, dt, H.MPI_REPLACE, O, Z, T, fetch)
        new, old, org = (gather(x, 0, q.offs, q.cnts, ext).reshape(-1, ext)
                         for x, q in ((got, T), (T.host, T), (O.host, O)))
        assert np.array_equal(new[:, m], org[:, m]) and np.array_equal(new[:, ~m], old[:, ~m])


# 8 ---------------------------------------------------------------------- sync forms
def test_sync_forms_return_with_the_results_visible(R, H, oracle):
    rng = np.random.default_rng(0x5EED1280)
    for op in (H.MPI_SUM, H.MPI_REPLACE, H.MPI_NO_OP):
        for fetch in (True, False):
            O, Z, T = fp64_sides(R, H, rng, TILE_LENS, O_LENS, Z_LENS)
            run_case(R, H, oracle, H.MPI_DOUBLE, op, O, Z, T, fetch, ('fp', 8, 'MPI_SUM'),
                     sync=True)
    O, Z, T = fp64_sides(R, H, rng, [300], [300], None)         # the contiguous path
    run_case(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, O, Z, T, True, ('fp', 8, 'MPI_SUM'), sync=True,
             prepare=False)
    # a host target is refused by the sync forms
    O, Z, T = fp64_sides(R, H, rng, TILE_LENS, O_LENS, Z_LENS)
    pin = torch.zeros(len(T.host), dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()
    assert R.accumulate_local_typed(O.v, O.plan, pin, T.plan, H.MPI_SUM,
                                    sync=True) == H.MPI_ERR_BUFFER
    assert R.get_accumulate_local_typed(O.v, O.plan, Z.v, Z.plan, pin, T.plan, H.MPI_SUM,
                                        sync=True) == H.MPI_ERR_BUFFER
    torch.cuda.synchronize()
    assert not pin.any() and (Z.P.bytes() == CANARY).all()
    for s in (O, Z, T):
        s.close()


# 9 -------------------------------------------------------------------- graph capture
def test_typed_calls_are_graph_capturable(R, H, oracle):
    """after prepare (target) and prepare_packed (origin, result): a typed
    accumulate and a typed fetch captured on one stream, no parallel branch;
    the capture runs nothing; three replays are three applications"""
    rng = np.random.default_rng(0x5EED1290)
    O, Z, T = fp64_sides(R, H, rng, TILE_LENS, O_LENS, Z_LENS)
    Ta = T.twin()
    ext, total = 8, 817
    try:
        assert T.plan.prepare() == 0
        assert O.plan.prepare_packed() == 0 and Z.plan.prepare_packed() == 0
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                assert typed_call(R, H.MPI_SUM, O, None, Ta, fetch=False) == 0
                assert typed_call(R, H.MPI_SUM, O, Z, T) == 0
        torch.cuda.synchronize()
        assert np.array_equal(T.P.bytes(), T.host) and np.array_equal(Ta.P.bytes(), T.host)
        assert np.array_equal(Z.P.bytes(), Z.host)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        packed = gather(O.host, 0, O.offs, O.cnts, ext)
        exp, two = T.host.copy(), None
        for k in range(3):
            if k == 2:
                two = exp.copy()
            assert oracle.reduce_local_iov(packed.copy(), exp, T.offs, T.cnts, H.MPI_DOUBLE,
                                           H.MPI_SUM) == 0
        assert np.array_equal(T.P.bytes(), exp) and np.array_equal(Ta.P.bytes(), exp)
        exp_z = Z.host.copy()
        exp_z[element_bytes(Z, ext, np.ones(ext, bool))] = \
            gather(two, 0, T.offs, T.cnts, ext).reshape(total, ext)
        assert np.array_equal(Z.P.bytes(), exp_z)
        assert np.array_equal(O.P.bytes(), O.host)
        assert all(x.P.guards_intact() for x in (O, Z, T, Ta))
        del g
    finally:
        torch.cuda.synchronize()
        for x in (O, Z, T):
            x.close()


# 10 -------------------------------------------------------------------- concurrency
def test_four_threads_on_one_set_of_plans(R, H, oracle):
    """each thread with a stream and buffers of its own, all released at once
    on one prepared set of plans"""
    rng = np.random.default_rng(0x5EED12A0)
    total = 4000
    mk = lambda span: make_operand(rng, 'fp', 8, span, 'MPI_DOUBLE')      # noqa: E731
    O0 = derived(R, rng, H.MPI_DOUBLE, 8, cuts_of(rng, total, 200), mk, total)
    Z0 = derived(R, rng, H.MPI_DOUBLE, 8, cuts_of(rng, total, 250), lambda s: canary(s, 8), total)
    T0 = derived(R, rng, H.MPI_DOUBLE, 8, cuts_of(rng, total, 300), mk, total)
    try:
        assert T0.plan.prepare() == 0
        assert O0.plan.prepare_packed() == 0 and Z0.plan.prepare_packed() == 0
        sets = []
        for _ in range(4):
            O, Z, T = O0.twin(), Z0.twin(), T0.twin()
            for s in (O, T):        # data of its own
                s.host = mk(len(s.host) // 8).view(np.uint8).reshape(-1).copy()
                s.P = Placed(s.host)
            sets.append((O, Z, T, T.twin()))
        streams = [torch.cuda.Stream() for _ in range(4)]
        torch.cuda.synchronize()
        gate, errs = threading.Barrier(4), []

        def work(k):
            try:
                O, Z, T, Ta = sets[k]
                gate.wait(timeout=30)
                for _ in range(3):
                    assert typed_call(R, H.MPI_SUM, O, Z, T, stream=streams[k]) == 0
                    assert typed_call(R, H.MPI_SUM, O, None, Ta, fetch=False,
                                      stream=streams[k]) == 0
            except Exception as e:      # noqa: BLE001
                errs.append(repr(e))
        ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        torch.cuda.synchronize()
        assert not errs, errs
        for O, Z, T, Ta in sets:
            packed = gather(O.host, 0, O.offs, O.cnts, 8)
            exp, two = T.host.copy(), None
            for k in range(3):
                if k == 2:
                    two = exp.copy()
                assert oracle.reduce_local_iov(packed.copy(), exp, T.offs, T.cnts, H.MPI_DOUBLE,
                                               H.MPI_SUM) == 0
            assert np.array_equal(T.P.bytes(), exp) and np.array_equal(Ta.P.bytes(), exp)
            exp_z = Z.host.copy()
            exp_z[element_bytes(Z, 8, np.ones(8, bool))] = \
                gather(two, 0, T.offs, T.cnts, 8).reshape(total, 8)
            assert np.array_equal(Z.P.bytes(), exp_z)
            assert np.array_equal(O.P.bytes(), O.host)
            assert all(x.P.guards_intact() for x in (O, Z, T, Ta))
    finally:
        torch.cuda.synchronize()
        for x in (O0, Z0, T0):
            x.close()


# 11 ---------------------------------------------------------------------- placement
def test_refused_calls_touch_nothing(R, H):
    rng = np.random.default_rng(0x5EED12B0)
    raw = [rng.integers(0, 256, 4096, dtype=np.uint8) for _ in range(3)]
    O, Z, T = (Placed(x) for x in raw)
    host = np.zeros(512, np.float64)
    torch.cuda.synchronize()
    with R.IovPlan.from_iov([0, 1024], [16, 16], H.MPI_DOUBLE) as p, \
            R.IovPlan.from_iov([0, 1024], [16, 16], H.MPIX_BFLOAT16) as pb, \
            R.IovPlan.from_iov([0, 1024], [16, 16], H.MPI_FLOAT) as pf, \
            R.IovPlan.from_iov([0, 1024], [16, 17], H.MPI_DOUBLE) as p9:
        for sync in (False, True):
            def fetch(o, op_, z, zp, t, tp, op=H.MPI_SUM):
                return R.get_accumulate_local_typed(o, op_, z, zp, t, tp, op, sync=sync)

            def acc(o, op_, t, tp, op=H.MPI_SUM):
                return R.accumulate_local_typed(o, op_, t, tp, op, sync=sync)
            # 1: no target plan
            f, tail = (R.lib().MPIX_Get_accumulate_local_typed, ()) if sync else \
                (R.lib().MPIX_Get_accumulate_local_typed_async, (None,))
            assert f(O.v.data_ptr(), p.handle, Z.v.data_ptr(), p.handle, T.v.data_ptr(), None,
                     H.as_c_int(H.MPI_SUM), *tail) == H.MPI_ERR_ARG
            # 2: the op
            assert fetch(O.v, p, Z.v, p, T.v, p, H.MPIX_EQUAL) == H.MPI_ERR_OP
            assert acc(O.v, p, T.v, p, H.MPI_BAND) == H.MPI_ERR_OP
            # 3: type and count of the origin's and the result's plan
            assert fetch(O.v, pf, Z.v, p, T.v, p) == H.MPI_ERR_TYPE
            assert fetch(O.v, p, Z.v, p9, T.v, p) == H.MPI_ERR_COUNT
            assert acc(O.v, p9, T.v, p) == H.MPI_ERR_COUNT
            # 5: a missing operand
            assert R.lib().MPIX_Accumulate_local_typed_async(
                None, p.handle, T.v.data_ptr(), p.handle, H.as_c_int(H.MPI_SUM), None) \
                == H.MPI_ERR_BUFFER
            # 6: the result inside the gap of the target's bounding range, the
            # origin's layout interleaved with the result's
            assert fetch(O.v, p, T.v[256:], None, T.v, p) == H.MPI_ERR_BUFFER
            assert acc(T.v[256:], None, T.v, p) == H.MPI_ERR_BUFFER
            assert fetch(O.v, p, O.v[512:], p, T.v, p) == H.MPI_ERR_BUFFER
            # 7: a legal pair without a kernel
            assert fetch(O.v, pb, Z.v, pb, T.v, pb, H.MPI_MAX) == H.MPI_ERR_TYPE
            assert acc(O.v, None, T.v, pb, H.MPI_PROD) == H.MPI_ERR_TYPE
            # 8: pageable operands
            assert fetch(host, p, Z.v, p, T.v, p) == H.MPI_ERR_BUFFER
            assert fetch(O.v, p, host, None, T.v, p) == H.MPI_ERR_BUFFER
            assert fetch(O.v, p, Z.v, p, host, p) == H.MPI_ERR_BUFFER
            assert acc(host, None, T.v, p) == H.MPI_ERR_BUFFER
            assert acc(O.v, p, host, p) == H.MPI_ERR_BUFFER
    torch.cuda.synchronize()
    for q, x in zip((O, Z, T), raw):
        assert np.array_equal(q.bytes(), x) and q.guards_intact()


def test_second_device(R, H, oracle):
    """one set of plans serving two devices: tables per device, prepared
    explicitly on one and at first use on the other"""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs 2 GPUs')
    rng = np.random.default_rng(0x5EED12C0)
    O0, Z0, T0 = fp64_sides(R, H, rng, TILE_LENS, O_LENS, Z_LENS)
    try:
        assert T0.plan.prepare(1) == 0
        assert O0.plan.prepare_packed(1) == 0 and Z0.plan.prepare_packed(1) == 0
        for d in (1, 0):
            with torch.cuda.device(d):
                sides = []
                for s in (O0, Z0, T0):
                    s.device = 'cuda:%d' % d
                    sides.append(s.twin())
                O, Z, T = sides
                O2, Z2, T2 = O.twin(), Z.twin(), T.twin()
                torch.cuda.synchronize(d)
                assert typed_call(R, H.MPI_SUM, O, Z, T) == 0
                composition(R, H, H.MPI_SUM, O2, Z2, T2, 8, 817)
                torch.cuda.synchronize(d)
                check(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, O, Z, T, O2, Z2, T2, True,
                      ('fp', 8, 'MPI_SUM'))
    finally:
        for s in (O0, Z0, T0):
            s.close()
