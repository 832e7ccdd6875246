"""Committed iov plans (MPIX_Iov_plan_*, MPIX_Reduce_local_plan*,
MPIX_Get_accumulate_local_plan*) on the GPU.

Every case checks three things:
  - the plan calls against oracle.reduce_local_iov[ec] on host copies;
  - the plan calls, bit for bit over the whole buffer, against the existing
    MPIX_Reduce_local_iov[ec]_async entry on a twin placed at the same byte
    offsets: the fetch form's target and the reduce form's target both;
  - for the fetch form, checks (a) to (e) of tests/test_getacc_iov_gpu.py.
"""
import threading

import numpy as np
import pytest
import torch

from tests.test_getacc_gpu import CANARY, Placed, _soft_operands, field_mask
from tests.test_getacc_iov_gpu import Case, gather, layout, many_runs, operands, MANY
from tests.test_gpu_parity import SWEEP, make_operand
from tests.test_iovec import pair_iov, random_pairs

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


class PlanCase(Case):
    """Case with the fetch going through a plan, and a third copy of target
    and origin for the plan's reduce form; the reduce-form twin of Case stays
    with the existing iov / iovec entry"""

    def __init__(self, R, H, dt, op, offs, cnts, tgt, org, plan=None, **place):
        super().__init__(R, H, dt, op, offs, cnts, tgt, org, **place)
        self.T3 = Placed(self.tgt)
        self.O3 = None if self.org is None else Placed(self.org, place.get('ooff', 0))
        self.own = plan is None
        if plan is not None:
            self.plan = plan
        elif self.iovec:
            self.plan = R.IovPlan.from_iovec(self.iovec[0], self.iovec[1], dt)
        else:
            self.plan = R.IovPlan.from_iov(self.offs, self.cnts, dt)

    def fetch(self, stream=None, sync=False):
        o = None if self.O is None else self.O.v
        return self.R.get_accumulate_local_plan(o, self.Z.v, self.T.v[self.base:], self.plan,
                                                self.op, stream=stream, sync=sync)

    def plan_reduce(self, stream=None, sync=False):
        """MPI_NO_OP without an origin: the reduce form would do nothing"""
        if self.O3 is None:
            return 0
        return self.R.reduce_local_plan(self.O3.v, self.T3.v[self.base:], self.plan, self.op,
                                        stream=stream, sync=sync)

    def issue(self, stream=None, sync=False):
        assert self.fetch(stream, sync) == 0
        assert self.plan_reduce(stream, sync) == 0
        assert self.reduce(None if sync else stream) == 0

    def check(self, oracle, parity=None):
        got = super().check(oracle, parity)
        assert np.array_equal(self.T3.bytes(), self.T2.bytes()), \
            'the reduce form differs from the iov entry'
        assert self.T3.guards_intact()
        if self.O3 is not None:
            assert np.array_equal(self.O3.bytes(), self.org) and self.O3.guards_intact()
        return got

    def close(self):
        if self.own:
            self.plan.close()


def plan_and_check(R, H, oracle, dt, op, offs, cnts, tgt, org, parity=None, prepare=True,
                   sync=False, runs=None, **place):
    c = PlanCase(R, H, dt, op, offs, cnts, tgt, org, **place)
    try:
        if runs is not None:
            assert c.plan.info()['runs'] == runs
        if prepare:
            assert c.plan.prepare() == 0
            assert c.plan.prepare() == 0        # idempotent
        torch.cuda.synchronize()
        c.issue(sync=sync)
        if not sync:
            torch.cuda.synchronize()
        else:
            torch.cuda.current_stream().synchronize()       # the twin's async entry only
        return c.check(oracle, parity)
    finally:
        torch.cuda.synchronize()
        c.close()


def fp64(rng, span, total):
    return make_operand(rng, 'fp', 8, span, 'MPI_DOUBLE'), make_operand(rng, 'fp', 8, total,
                                                                        'MPI_DOUBLE')


# 1 ------------------------------------------------------------------- tile edges
TILE_LENS = [255, 1, 1, 255, 300, 5]


def tile_edges(rng, reps=1):
    lens = TILE_LENS * reps
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1].tolist()
    assert starts[:6] == [0, 255, 256, 257, 512, 812] and sum(TILE_LENS) % 256
    offs, span = layout(rng, lens, 8)           # gaps of 1 to 5 elements: nothing merges
    return lens, offs, span


def test_tile_edges(R, H, oracle):
    """run starts at packed indices 255, 256, 257 and 512, a partial last tile"""
    rng = np.random.default_rng(0x5EED0D10)
    lens, offs, span = tile_edges(rng)
    tgt, org = fp64(rng, span, sum(lens))
    plan_and_check(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, offs, lens, tgt, org,
                   ('fp', 8, 'MPI_SUM'), runs=6)
    plan_and_check(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, offs, lens, tgt, org,
                   ('fp', 8, 'MPI_SUM'), ooff=8, roff=16, prepare=False)


def test_many_runs_per_tile(R, H, oracle):
    rng = np.random.default_rng(0x5EED0D11)
    lens = [1] * 700
    offs, span = layout(rng, lens, 8)
    tgt, org = fp64(rng, span, 700)
    plan_and_check(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, offs, lens, tgt, org,
                   ('fp', 8, 'MPI_SUM'), runs=700)


def test_one_run_across_many_tiles(R, H, oracle):
    rng = np.random.default_rng(0x5EED0D12)
    for lens in ([3, 1500], [1500, 3]):
        offs, span = layout(rng, lens, 8)
        tgt, org = fp64(rng, span, sum(lens))
        plan_and_check(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, offs, lens, tgt, org,
                       ('fp', 8, 'MPI_SUM'), runs=2)


def test_capped_grid(R, H, oracle):
    """max_grid = 2: the tile-edges case (one block walks all four tiles), and
    three of it in a row, where each of the two blocks takes every other tile"""
    rng = np.random.default_rng(0x5EED0D13)
    before = R.get_launch()
    assert R.set_launch(before['block'], 2) == 0
    try:
        for reps in (1, 3):
            lens, offs, span = tile_edges(rng, reps)
            assert reps == 1 or sum(lens) > 2 * 1024
            tgt, org = fp64(rng, span, sum(lens))
            for op, o in ((H.MPI_SUM, org), (H.MPI_REPLACE, org), (H.MPI_NO_OP, None)):
                plan_and_check(R, H, oracle, H.MPI_DOUBLE, op, offs, lens, tgt, o,
                               ('fp', 8, 'MPI_SUM'), runs=6 * reps)
    finally:
        assert R.set_launch(before['block'], before['max_grid']) == 0
    assert R.get_launch() == before


# 2 ------------------------------------------------------------ order and residues
def test_two_residues_shuffled_order_negative_offsets(R, H, oracle):
    """the shape of test_shuffled_order_negative_offsets_and_residues: target
    positions shuffled against the packed order, offsets below the target
    pointer, two residue groups whose packed positions alternate"""
    rng = np.random.default_rng(0x5EED0D20)
    lens = [int(x) for x in rng.integers(0, 12, 90)]
    lens[10], lens[11], lens[40] = 64, 300, 130
    slots, span = layout(rng, lens, 8, gap=(3, 6))
    order = rng.permutation(len(lens))
    shifts = [0, 4, -12]
    base = (span // 2) * 8
    offs = [slots[j] + 8 + shifts[i % 3] - base for i, j in enumerate(order)]
    cnts = [lens[j] for j in order]
    assert min(offs) < 0 < max(offs)
    assert {o % 8 for o, c in zip(offs, cnts) if c} == {0, 4}
    tgt, org = fp64(rng, span + 2, sum(cnts))
    with R.IovPlan.from_iov(offs, cnts, H.MPI_DOUBLE) as p:
        i = p.info()
        assert i['groups'] == 2 and i['lo_byte'] < 0 and i['elements'] == sum(cnts)
    plan_and_check(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, offs, cnts, tgt, org,
                   ('fp', 8, 'MPI_SUM'), base=base)
    desc = sorted(range(len(lens)), key=lambda j: -slots[j])
    plan_and_check(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, [slots[j] - base for j in desc],
                   [lens[j] for j in desc], tgt, org, ('fp', 8, 'MPI_SUM'), base=base, roff=8)


# 3 ------------------------------------------------------------------------ merging
def test_merged_and_unmerged_twins_give_identical_bits(R, H, oracle):
    """one layout given whole and cut into adjacent pieces (zero-length ones in
    between): the same plan after the merge, the same bits -- and the bits of
    the iov entry, which walks the pieces one by one"""
    rng = np.random.default_rng(0x5EED0D30)
    lens = [int(x) for x in rng.integers(1, 400, 12)]
    offs, span = layout(rng, lens, 4)
    poffs, pcnts = [], []
    for o, n in zip(offs, lens):
        cuts = sorted(set(rng.integers(0, n + 1, 5).tolist()) | {0, n})
        for a, b in zip(cuts, cuts[1:]):
            poffs += [o + 4 * a, o + 4 * b]     # the piece, then an empty run at its end
            pcnts += [b - a, 0]
    assert len(poffs) > 3 * len(lens)
    tgt = make_operand(rng, 'fp', 4, span, 'MPI_FLOAT')
    org = make_operand(rng, 'fp', 4, sum(lens), 'MPI_FLOAT')
    for op in (H.MPI_PROD, H.MPI_REPLACE):
        whole = plan_and_check(R, H, oracle, H.MPI_FLOAT, op, offs, lens, tgt, org,
                               ('fp', 4, 'MPI_PROD'), runs=len(lens))
        pieces = plan_and_check(R, H, oracle, H.MPI_FLOAT, op, poffs, pcnts, tgt, org,
                                ('fp', 4, 'MPI_PROD'), runs=len(lens))
        assert np.array_equal(whole, pieces)


# 4 ---------------------------------------------------------------- single-run plans
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('dtname,size,off', [('MPI_FLOAT', 4, 4), ('MPI_DOUBLE', 8, 8)],
                         ids=['fp32-4mod16', 'fp64-8mod16'])
def test_single_run_plans(R, H, oracle, dtname, size, off, n):
    """one run after merging: the contiguous entries' path with the target at
    its run offset, off the 16-byte phase"""
    dt = getattr(H, dtname)
    rng = np.random.default_rng(0x5EED0D40 + 16 * n + size)
    tgt = make_operand(rng, 'fp', size, n + 8, dtname)
    org = make_operand(rng, 'fp', size, n, dtname)
    half = n // 2
    # given as two adjacent runs (when n > 1), so the single run is a merged one
    offs, cnts = ([off, off + half * size], [half, n - half]) if half else ([off], [n])
    for opname, o, prep in (('MPI_SUM', org, True), ('MPI_MAX', org, False),
                            ('MPI_REPLACE', org, True), ('MPI_NO_OP', None, True)):
        c = plan_and_check(R, H, oracle, dt, getattr(H, opname), offs, cnts, tgt, o,
                           ('fp', size, opname), runs=1, prepare=prep, ooff=size, roff=2 * size)
        assert len(c) == (n + 8) * size
    with R.IovPlan.from_iov(offs, cnts, dt) as p:
        assert p.info()['table_bytes'] == 0 and p.info()['lo_byte'] == off


def test_single_run_double_int_iovec(R, H, oracle):
    """37 contiguous MPI_DOUBLE_INT elements as their raw iov (74 segments)"""
    dt = H.MPI_DOUBLE_INT
    rng = np.random.default_rng(0x5EED0D41)
    tgt, org = random_pairs(rng, dt, 40), random_pairs(rng, dt, 37)
    tgt['v'][rng.integers(0, 40, 6)] = np.nan
    org['v'][rng.integers(0, 37, 6)] = np.nan
    pos = list(range(2, 39))
    ioffs, ilens = pair_iov(dt, pos, False)
    assert len(ioffs) == 74
    for op in (H.MPI_MAXLOC, H.MPI_MINLOC, H.MPI_REPLACE, H.MPI_NO_OP):
        got = plan_and_check(R, H, oracle, dt, op, [p * 16 for p in pos], [1] * 37, tgt, org,
                             runs=1, iovec=(ioffs, ilens))
        pad = ~np.tile(field_mask(H, dt, 16), 40)
        assert np.array_equal(got[pad], tgt.view(np.uint8)[pad])


# 5 --------------------------------------------------------------------- type sweep
SWEEP_LENS = [1, 255, 17, 0, 68, 259]       # 600 elements, run starts at 256 and 273


@pytest.mark.parametrize('dtname,opname,kind,size', SWEEP,
                         ids=['%s-%s' % (s[0], s[1]) for s in SWEEP])
def test_every_pair(R, H, oracle, dtname, opname, kind, size):
    dt, op = getattr(H, dtname), getattr(H, opname)
    ext = R.datatype_extent(dt)
    rng = np.random.default_rng((0x5EED0D50 * 31 + dt * 7 + op) & 0xffffffff)
    offs, span = layout(rng, SWEEP_LENS, ext)
    tgt, org = operands(H, rng, dtname, kind, size, span, sum(SWEEP_LENS))
    plan_and_check(R, H, oracle, dt, op, offs, SWEEP_LENS, tgt, org, (kind, size, opname),
                   runs=5, ooff=ext)


@pytest.mark.parametrize('dtname', ['MPI_COMPLEX32', 'MPI_C_LONG_DOUBLE_COMPLEX'])
def test_wide_complex_products(R, H, oracle, dtname):
    """the split combiners' full apply, special values and real-valued operands
    (every product off its fast path) included"""
    dt = getattr(H, dtname)
    rng = np.random.default_rng(0x5EED0D51 + (dt & 0xff))
    offs, span = layout(rng, SWEEP_LENS, 32)
    for zero_im in (False, True):
        tgt, org = _soft_operands(H, rng, dtname, span, zero_im)
        plan_and_check(R, H, oracle, dt, H.MPI_PROD, offs, SWEEP_LENS, tgt.reshape(-1)[:span * 32],
                       org.reshape(-1)[:600 * 32], runs=5)


# 6 ------------------------------------------------------------- NO_OP and REPLACE
@pytest.mark.parametrize('dtname,kind,size', MANY, ids=[m[0] for m in MANY])
def test_no_op_and_replace(R, H, oracle, dtname, kind, size):
    rng = np.random.default_rng(0x5EED0D60 + len(dtname))
    dt, ext, lens, offs, tgt, org = many_runs(R, H, rng, dtname, kind, size)
    got = plan_and_check(R, H, oracle, dt, H.MPI_NO_OP, offs, lens, tgt, None, roff=ext)
    assert np.array_equal(got, tgt)
    got = plan_and_check(R, H, oracle, dt, H.MPI_REPLACE, offs, lens, tgt, org, ooff=ext)
    m = np.tile(field_mask(H, dt, ext), sum(lens))
    assert np.array_equal(gather(got, 0, offs, lens, ext)[m], org[m])
    assert np.array_equal(gather(got, 0, offs, lens, ext)[~m], gather(tgt, 0, offs, lens, ext)[~m])
    # the reduce form's MPI_NO_OP leaves the target alone (a source it must be given)
    got = plan_and_check(R, H, oracle, dt, H.MPI_NO_OP, offs, lens, tgt, org)
    assert np.array_equal(got, tgt)


# 7 ---------------------------------------------------------------------- sync forms
def test_sync_forms_return_with_the_results_visible(R, H, oracle):
    rng = np.random.default_rng(0x5EED0D70)
    lens, offs, span = tile_edges(rng)
    tgt, org = fp64(rng, span, sum(lens))
    for op, o in ((H.MPI_SUM, org), (H.MPI_REPLACE, org), (H.MPI_NO_OP, None)):
        plan_and_check(R, H, oracle, H.MPI_DOUBLE, op, offs, lens, tgt, o, ('fp', 8, 'MPI_SUM'),
                       sync=True)
    plan_and_check(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, [8], [300], tgt, org,
                   ('fp', 8, 'MPI_SUM'), sync=True, prepare=False)      # a single run
    # a host target is refused by the sync forms
    with R.IovPlan.from_iov(offs, lens, H.MPI_DOUBLE) as p:
        O, Z = Placed(org), Placed(org)
        pin = torch.zeros(span * 8, dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()
        assert R.reduce_local_plan(O.v, pin, p, H.MPI_SUM, sync=True) == H.MPI_ERR_BUFFER
        assert R.get_accumulate_local_plan(O.v, Z.v, pin, p, H.MPI_SUM,
                                           sync=True) == H.MPI_ERR_BUFFER
        assert not pin.any()


# 8 ------------------------------------------------------------ reuse and concurrency
def test_one_plan_three_calls(R, H, oracle):
    rng = np.random.default_rng(0x5EED0D80)
    lens, offs, span = tile_edges(rng)
    with R.IovPlan.from_iov(offs, lens, H.MPI_DOUBLE) as p:
        assert p.prepare() == 0
        cases = []
        for op in (H.MPI_SUM, H.MPI_MAX, H.MPI_PROD):
            tgt, org = fp64(rng, span, sum(lens))
            cases.append(PlanCase(R, H, H.MPI_DOUBLE, op, offs, lens, tgt, org, plan=p))
        torch.cuda.synchronize()
        for c in cases:
            c.issue()
        torch.cuda.synchronize()
        for c, opname in zip(cases, ('MPI_SUM', 'MPI_MAX', 'MPI_PROD')):
            c.check(oracle, ('fp', 8, opname))


def test_four_threads_on_one_plan(R, H, oracle):
    """each thread with a stream of its own, all released at once on one
    prepared plan"""
    rng = np.random.default_rng(0x5EED0D81)
    lens = [int(x) for x in rng.integers(1, 40, 300)]
    offs, span = layout(rng, lens, 8)
    with R.IovPlan.from_iov(offs, lens, H.MPI_DOUBLE) as p:
        assert p.prepare() == 0
        cases = [PlanCase(R, H, H.MPI_DOUBLE, H.MPI_SUM, offs, lens, *fp64(rng, span, sum(lens)),
                          plan=p) for _ in range(4)]
        streams = [torch.cuda.Stream() for _ in range(4)]
        torch.cuda.synchronize()
        gate, errs = threading.Barrier(4), []

        def work(k):
            try:
                gate.wait(timeout=30)
                for _ in range(3):
                    assert cases[k].fetch(streams[k]) == 0
                    assert cases[k].plan_reduce(streams[k]) == 0
            except Exception as e:      # noqa: BLE001
                errs.append(repr(e))
        ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        torch.cuda.synchronize()
        assert not errs, errs
        # three applications each: the oracle and the iov entry three times over
        for c in cases:
            exp = c.tgt.copy()
            for _ in range(3):
                assert c.reduce() == 0
                assert oracle.reduce_local_iov(c.org.copy(), exp, offs, lens, H.MPI_DOUBLE,
                                               H.MPI_SUM) == 0
            torch.cuda.synchronize()
            for got in (c.T.bytes(), c.T3.bytes()):
                assert np.array_equal(got, c.T2.bytes())
                assert np.array_equal(got, exp)
            assert c.T.guards_intact() and c.T3.guards_intact() and c.Z.guards_intact()


# 9 ------------------------------------------------------------------- graph capture
def test_plan_calls_are_graph_capturable(R, H, oracle):
    """after prepare, a plan reduce and a plan fetch captured on one stream, as
    test_async_is_graph_capturable does; the capture runs nothing; three
    replays are three applications.  Once with the indexed tables, once with a
    plan of one run (the contiguous entries' path, off the 16-byte phase)."""
    rng = np.random.default_rng(0x5EED0D90)
    lens, offs, span = tile_edges(rng)
    for lens, offs, span in ((lens, offs, span), ([300, 217], [8, 8 + 300 * 8], 520)):
        capture_and_replay(R, H, oracle, rng, lens, offs, span)


def capture_and_replay(R, H, oracle, rng, lens, offs, span):
    a, b = rng.uniform(-1, 1, span), rng.uniform(-1, 1, sum(lens))
    ab = a.view(np.uint8)
    with R.IovPlan.from_iov(offs, lens, H.MPI_DOUBLE) as p:
        assert p.prepare() == 0
        assert (p.info()['runs'] == 1) == (len(lens) == 2)
        Tr, Tf, O = Placed(a), Placed(a), Placed(b)
        Z = Placed(np.full(sum(lens) * 8, CANARY, np.uint8))
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                assert R.reduce_local_plan(O.v, Tr.v, p, H.MPI_SUM) == 0
                assert R.get_accumulate_local_plan(O.v, Z.v, Tf.v, p, H.MPI_SUM) == 0
        torch.cuda.synchronize()
        assert np.array_equal(Tr.bytes(), ab) and np.array_equal(Tf.bytes(), ab)
        assert (Z.bytes() == CANARY).all()
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        exp, two = a.copy(), None
        for k in range(3):
            if k == 2:
                two = exp.copy()
            assert oracle.reduce_local_iov(b.copy(), exp, offs, lens, H.MPI_DOUBLE, H.MPI_SUM) == 0
        assert np.array_equal(Tr.bytes(), exp.view(np.uint8))
        assert np.array_equal(Tf.bytes(), exp.view(np.uint8))
        assert np.array_equal(Z.bytes(), gather(two.view(np.uint8), 0, offs, lens, 8))
        assert Tr.guards_intact() and Tf.guards_intact() and Z.guards_intact()
        del g


# 10 ---------------------------------------------------------------------- placement
def test_refused_calls_touch_nothing(R, H):
    rng = np.random.default_rng(0x5EED0DA0)
    raw = [rng.integers(0, 256, 4096, dtype=np.uint8) for _ in range(3)]
    O, Z, T = (Placed(x) for x in raw)
    host = np.zeros(512, np.float64)
    torch.cuda.synchronize()
    with R.IovPlan.from_iov([0, 1024], [16, 16], H.MPI_DOUBLE) as p, \
            R.IovPlan.from_iov([0, 1024], [16, 16], H.MPIX_BFLOAT16) as pb:
        for sync in (False, True):
            # pageable operands
            assert R.get_accumulate_local_plan(host, Z.v, T.v, p, H.MPI_SUM,
                                               sync=sync) == H.MPI_ERR_BUFFER
            assert R.get_accumulate_local_plan(O.v, host, T.v, p, H.MPI_SUM,
                                               sync=sync) == H.MPI_ERR_BUFFER
            assert R.get_accumulate_local_plan(O.v, Z.v, host, p, H.MPI_SUM,
                                               sync=sync) == H.MPI_ERR_BUFFER
            assert R.reduce_local_plan(host, T.v, p, H.MPI_SUM, sync=sync) == H.MPI_ERR_BUFFER
            assert R.reduce_local_plan(O.v, host, p, H.MPI_SUM, sync=sync) == H.MPI_ERR_BUFFER
            # the result inside the gap of the bounding range; origin over result
            assert R.get_accumulate_local_plan(O.v, T.v[256:], T.v, p, H.MPI_SUM,
                                               sync=sync) == H.MPI_ERR_BUFFER
            assert R.reduce_local_plan(T.v[256:], T.v, p, H.MPI_SUM, sync=sync) == H.MPI_ERR_BUFFER
            assert R.get_accumulate_local_plan(O.v, O.v[255:], T.v, p, H.MPI_SUM,
                                               sync=sync) == H.MPI_ERR_BUFFER
            assert R.get_accumulate_local_plan(O.v, Z.v, T.v, p, H.MPIX_EQUAL,
                                               sync=sync) == H.MPI_ERR_OP
            assert R.get_accumulate_local_plan(O.v, Z.v, T.v, pb, H.MPI_MAX,
                                               sync=sync) == H.MPI_ERR_TYPE
            assert R.reduce_local_plan(O.v, T.v, pb, H.MPI_PROD, sync=sync) == H.MPI_ERR_TYPE
    torch.cuda.synchronize()
    for q, x in zip((O, Z, T), raw):
        assert np.array_equal(q.bytes(), x) and q.guards_intact()


def test_second_device(R, H, oracle):
    """one plan serving two devices: tables per device, prepared explicitly on
    one and at first use on the other"""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs 2 GPUs')
    rng = np.random.default_rng(0x5EED0DB0)
    lens, offs, span = tile_edges(rng)
    tgt, org = fp64(rng, span, sum(lens))
    exp = tgt.copy()
    assert oracle.reduce_local_iov(org.copy(), exp, offs, lens, H.MPI_DOUBLE, H.MPI_SUM) == 0
    with R.IovPlan.from_iov(offs, lens, H.MPI_DOUBLE) as p:
        assert p.prepare(1) == 0
        for d in (1, 0):
            with torch.cuda.device(d):
                T, T3, O = (Placed(x, device='cuda:%d' % d) for x in (tgt, tgt, org))
                Z = Placed(np.full(sum(lens) * 8, CANARY, np.uint8), device='cuda:%d' % d)
                torch.cuda.synchronize(d)
                assert R.get_accumulate_local_plan(O.v, Z.v, T.v, p, H.MPI_SUM) == 0
                assert R.reduce_local_plan(O.v, T3.v, p, H.MPI_SUM, sync=True) == 0
                torch.cuda.synchronize(d)
                for q in (T, T3):
                    assert np.array_equal(q.bytes(), exp.view(np.uint8)) and q.guards_intact()
                assert np.array_equal(Z.bytes(), gather(tgt.view(np.uint8), 0, offs, lens, 8))
