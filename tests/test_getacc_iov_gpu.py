"""The fused get-accumulate on iov / iovec targets
(MPIX_Get_accumulate_local_iov_async, MPIX_Get_accumulate_local_iovec_async)
on the GPU.

Every fetch case checks five things:
  (a) `result` is the gather of the target's bytes from before the call, type
      map only, the result's padding still holding its canary;
  (b) the target equals oracle.reduce_local_iov / reduce_local_iovec on host
      copies: its run elements under the parity rule of tests/test_gpu_parity.py
      (compare), every byte outside the runs unchanged;
  (c) the target is bit-identical, over its whole extent including gaps, to
      what MPIX_Reduce_local_iov[ec]_async leaves on a copy placed at the same
      byte offsets;
  (d) the origin is unchanged;
  (e) the guard bytes of all three buffers are intact.
"""
import numpy as np
import pytest
import torch

from tests.test_getacc_gpu import CANARY, Placed, _soft_operands, expected_result, field_mask
from tests.test_gpu_parity import SWEEP, compare, make_operand
from tests.test_iovec import PAIRS, pair_iov, random_pairs

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


def gather(buf, base, offs, cnts, ext):
    """the runs' bytes of `buf` (target pointer at byte `base`), in run order"""
    parts = [buf[base + o:base + o + c * ext] for o, c in zip(offs, cnts) if c]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def run_mask(nbytes, base, offs, cnts, ext):
    m = np.zeros(nbytes, bool)
    for o, c in zip(offs, cnts):
        m[base + o:base + o + c * ext] = True
    return m


class Case:
    """one fetch call and its reduce-form twin, placed but not yet issued"""

    def __init__(self, R, H, dt, op, offs, cnts, tgt, org, base=0, iovec=None, ooff=0, roff=0):
        self.R, self.H, self.dt, self.op = R, H, dt, op
        self.offs, self.cnts, self.base, self.iovec = list(offs), list(cnts), base, iovec
        self.ext = R.datatype_extent(dt)
        self.total = sum(cnts)
        self.tgt = np.ascontiguousarray(tgt).view(np.uint8).reshape(-1)
        self.org = None if org is None else \
            np.ascontiguousarray(org).view(np.uint8).reshape(-1)[:self.total * self.ext]
        self.T, self.T2 = Placed(self.tgt), Placed(self.tgt)
        self.Z = Placed(np.full(self.total * self.ext, CANARY, np.uint8), roff)
        self.O = self.O2 = None
        if self.org is not None:
            self.O, self.O2 = Placed(self.org, ooff), Placed(self.org, ooff)

    def fetch(self, stream=None):
        o = None if self.O is None else self.O.v
        if self.iovec:
            return self.R.get_accumulate_local_iovec(o, self.Z.v, self.T.v[self.base:],
                                                     self.iovec[0], self.iovec[1], self.dt,
                                                     self.op, stream=stream)
        return self.R.get_accumulate_local_iov(o, self.Z.v, self.T.v[self.base:], self.offs,
                                               self.cnts, self.dt, self.op, stream=stream)

    def reduce(self, stream=None):
        """the reduce form on the twin; MPI_NO_OP with no origin leaves it as it is"""
        if self.O2 is None:
            return 0
        if self.iovec:
            return self.R.reduce_local_iovec_async(self.O2.v, self.T2.v[self.base:],
                                                   self.iovec[0], self.iovec[1], self.dt, self.op,
                                                   stream=stream)
        return self.R.reduce_local_iov_async(self.O2.v, self.T2.v[self.base:], self.offs,
                                             self.cnts, self.dt, self.op, stream=stream)

    def check(self, oracle, parity=None):
        """after synchronising: (a)-(e); returns the target's bytes"""
        H, ext = self.H, self.ext
        got = self.T.bytes()
        before = gather(self.tgt, self.base, self.offs, self.cnts, ext)
        assert np.array_equal(self.Z.bytes(), expected_result(H, self.dt, ext, before,
                                                              self.total)), '(a) result'
        exp = self.tgt.copy()
        org = np.zeros(max(self.total * ext, 1), np.uint8) if self.org is None else self.org.copy()
        if self.iovec:
            assert oracle.reduce_local_iovec(org, exp[self.base:], self.iovec[0], self.iovec[1],
                                             self.dt, self.op) == 0
        else:
            assert oracle.reduce_local_iov(org, exp[self.base:], self.offs, self.cnts, self.dt,
                                           self.op) == 0
        if parity:
            kind, size, opname = parity
            assert compare(gather(got, self.base, self.offs, self.cnts, ext),
                           gather(exp, self.base, self.offs, self.cnts, ext), kind, size, opname,
                           ext) == 0, '(b) oracle'
            gaps = ~run_mask(len(got), self.base, self.offs, self.cnts, ext)
            assert np.array_equal(got[gaps], self.tgt[gaps]), '(b) a gap byte changed'
        else:
            assert np.array_equal(got, exp), '(b) oracle'
        assert np.array_equal(got, self.T2.bytes()), '(c) target differs from the reduce form'
        if self.O is not None:
            assert np.array_equal(self.O.bytes(), self.org), '(d) origin changed'
            assert self.O.guards_intact(), '(e) origin guards'
        assert self.T.guards_intact() and self.Z.guards_intact(), '(e) guard bytes'
        return got


def fetch_iov_and_check(R, H, oracle, dt, op, offs, cnts, tgt, org, parity=None, **place):
    c = Case(R, H, dt, op, offs, cnts, tgt, org, **place)
    torch.cuda.synchronize()
    assert c.fetch() == 0
    assert c.reduce() == 0
    torch.cuda.synchronize()
    return c.check(oracle, parity)


def layout(rng, lens, ext, gap=(1, 6)):
    """runs of `lens` elements laid out in order with gaps of gap[0]..gap[1]-1
    elements: (byte offsets, span in elements)"""
    offs, pos = [], 0
    for n in lens:
        pos += int(rng.integers(*gap))
        offs.append(pos * ext)
        pos += n
    return offs, pos + 1


def operands(H, rng, dtname, kind, size, span, total):
    if kind == 'soft':
        tgt, org = _soft_operands(H, rng, dtname, max(span, total), False)
        return tgt.reshape(-1)[:span * 32], org.reshape(-1)[:total * 32]
    return make_operand(rng, kind, size, span, dtname), make_operand(rng, kind, size, total, dtname)


# 1 ---------------------------------------------------------- run-length edges
EDGE_LENS = [0, 1, 2, 3, 63, 64, 65, 127, 129, 300]
EDGE_TYPES = [('MPI_INT8_T', 'MPI_MAX', 'int', 1), ('MPI_INT16_T', 'MPI_BXOR', 'int', 2),
              ('MPI_FLOAT', 'MPI_SUM', 'fp', 4), ('MPI_DOUBLE', 'MPI_PROD', 'fp', 8),
              ('MPI_INTEGER16', 'MPI_SUM', 'int', 16),
              ('MPI_C_DOUBLE_COMPLEX', 'MPI_PROD', 'cplx', 8),
              ('MPI_C_LONG_DOUBLE_COMPLEX', 'MPI_SUM', 'soft', None),
              ('MPI_LONG_DOUBLE_INT', 'MPI_MAXLOC', 'soft', None)]


def edge_runs(rng):
    """every edge length twice in shuffled order around a stretch of 72 runs of
    one element (a wave spanning 64 runs): 1,980 elements"""
    a, b = list(EDGE_LENS), list(EDGE_LENS)
    rng.shuffle(a)
    rng.shuffle(b)
    lens = a + [1] * 72 + b + [200, 200]
    assert sum(lens) == 1980
    return [int(x) for x in lens]


@pytest.mark.parametrize('dtname,opname,kind,size', EDGE_TYPES, ids=[t[0] for t in EDGE_TYPES])
def test_run_length_edges(R, H, oracle, dtname, opname, kind, size):
    """a wave inside one run, straddling two, straddling 64, zero-length runs
    in between; origin and result on and off the target's phase"""
    dt, op = getattr(H, dtname), getattr(H, opname)
    ext = R.datatype_extent(dt)
    rng = np.random.default_rng(0x5EED0C00 + ext + len(dtname))
    lens = edge_runs(rng)
    offs, span = layout(rng, lens, ext)
    tgt, org = operands(H, rng, dtname, kind, size, span, sum(lens))
    parity = None if kind == 'soft' else (kind, size, opname)
    fetch_iov_and_check(R, H, oracle, dt, op, offs, lens, tgt, org, parity)
    fetch_iov_and_check(R, H, oracle, dt, op, offs, lens, tgt, org, parity, ooff=ext, roff=2 * ext)


# 2 --------------------------------------------------------- order and residues
def test_shuffled_order_negative_offsets_and_residues(R, H, oracle):
    """fp64 runs whose target positions are shuffled against the packed order,
    at offsets below the target pointer, shifted by 0, 4 and -12 bytes in turn:
    two residue groups whose packed positions alternate, so the packed index of
    the result is src_off, not the group's prefix"""
    rng = np.random.default_rng(0x5EED0C10)
    lens = [int(x) for x in rng.integers(0, 12, 90)]
    lens[10], lens[11], lens[40] = 64, 70, 130
    slots, span = layout(rng, lens, 8, gap=(3, 6))      # room for the -12 / +4 byte shifts
    order = rng.permutation(len(lens))
    assert (np.diff(order) < 0).any()
    shifts = [0, 4, -12]
    base = (span // 2) * 8
    offs = [slots[j] + 8 + shifts[i % 3] - base for i, j in enumerate(order)]
    cnts = [lens[j] for j in order]
    assert min(offs) < 0 < max(offs)
    assert {o % 8 for o, c in zip(offs, cnts) if c} == {0, 4}
    tgt = make_operand(rng, 'fp', 8, span + 2, 'MPI_DOUBLE')
    org = make_operand(rng, 'fp', 8, sum(cnts), 'MPI_DOUBLE')
    fetch_iov_and_check(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, offs, cnts, tgt, org,
                        ('fp', 8, 'MPI_SUM'), base=base)
    # descending target offsets, ascending packed order
    desc = sorted(range(len(lens)), key=lambda j: -slots[j])
    offs = [slots[j] - base for j in desc]
    cnts = [lens[j] for j in desc]
    fetch_iov_and_check(R, H, oracle, H.MPI_DOUBLE, H.MPI_SUM, offs, cnts, tgt, org,
                        ('fp', 8, 'MPI_SUM'), base=base, roff=8)


# 3 ------------------------------------------ padded pairs through the iovec form
PAIR_NAMES = ['MPI_DOUBLE_INT', 'MPI_LONG_INT', 'MPI_SHORT_INT', 'MPI_FLOAT_INT']


@pytest.mark.parametrize('opname', ['MPI_MAXLOC', 'MPI_MINLOC', 'MPI_REPLACE', 'MPI_NO_OP'])
@pytest.mark.parametrize('merge', [False, True], ids=['split', 'merged'])
@pytest.mark.parametrize('dtname', PAIR_NAMES)
def test_padded_pairs_through_iovec(R, H, oracle, dtname, merge, opname):
    """{value, int} segments gathered into elements; the result's padding (the
    canary, (a)) and the target's (whole-buffer equality with the oracle, (b))
    both stay"""
    dt, op = getattr(H, dtname), getattr(H, opname)
    ext = PAIRS[dt][3]
    rng = np.random.default_rng(0x5EED0C20 + (dt & 0xff) * 8 + merge)
    n = 100
    pos = sorted(set(rng.integers(0, 2 * n, n).tolist()) | set(range(30, 50)))
    tgt, org = random_pairs(rng, dt, 2 * n), random_pairs(rng, dt, len(pos))
    if PAIRS[dt][0].startswith('<f'):
        tgt['v'][rng.integers(0, 2 * n, 12)] = np.nan
        org['v'][rng.integers(0, len(pos), 8)] = np.nan
    ioffs, ilens = pair_iov(dt, pos, merge)
    offs, cnts = [p * ext for p in pos], [1] * len(pos)
    if dt == H.MPI_FLOAT_INT and not merge:
        # size == extent: not a pairtype, a 4-byte segment is a partial element
        c = Case(R, H, dt, op, offs, cnts, tgt, org, iovec=(ioffs, ilens))
        torch.cuda.synchronize()
        assert c.fetch() == H.MPI_ERR_ARG
        torch.cuda.synchronize()
        assert np.array_equal(c.T.bytes(), c.tgt) and np.array_equal(c.O.bytes(), c.org)
        assert (c.Z.bytes() == CANARY).all()
        return
    got = fetch_iov_and_check(R, H, oracle, dt, op, offs, cnts, tgt, org, iovec=(ioffs, ilens))
    pad = ~np.tile(field_mask(H, dt, ext), 2 * n)
    assert np.array_equal(got[pad], tgt.view(np.uint8)[pad])


# 4 ----------------------------------------------------------- NO_OP and REPLACE
MANY = [('MPI_FLOAT', 'fp', 4), ('MPI_INT8_T', 'int', 1),
        ('MPI_DOUBLE_INT', ('pair', '<f8', '<i4', 16, 8), None)]


def many_runs(R, H, rng, dtname, kind, size):
    dt = getattr(H, dtname)
    ext = R.datatype_extent(dt)
    lens = [int(x) for x in rng.integers(0, 7, 330)]
    offs, span = layout(rng, lens, ext, gap=(0, 4))
    tgt = make_operand(rng, kind, size, span, dtname)
    org = make_operand(rng, kind, size, sum(lens), dtname)
    return dt, ext, lens, offs, tgt, org


@pytest.mark.parametrize('dtname,kind,size', MANY, ids=[m[0] for m in MANY])
def test_no_op_gathers_330_runs_without_an_origin(R, H, oracle, dtname, kind, size):
    rng = np.random.default_rng(0x5EED0C30 + len(dtname))
    dt, ext, lens, offs, tgt, _ = many_runs(R, H, rng, dtname, kind, size)
    got = fetch_iov_and_check(R, H, oracle, dt, H.MPI_NO_OP, offs, lens, tgt, None, roff=ext)
    assert np.array_equal(got, tgt)


@pytest.mark.parametrize('dtname,kind,size', MANY, ids=[m[0] for m in MANY])
def test_replace_swaps_330_runs(R, H, oracle, dtname, kind, size):
    rng = np.random.default_rng(0x5EED0C40 + len(dtname))
    dt, ext, lens, offs, tgt, org = many_runs(R, H, rng, dtname, kind, size)
    got = fetch_iov_and_check(R, H, oracle, dt, H.MPI_REPLACE, offs, lens, tgt, org, ooff=ext)
    m = np.tile(field_mask(H, dt, ext), sum(lens))
    assert np.array_equal(gather(got, 0, offs, lens, ext)[m], org[m])
    assert np.array_equal(gather(got, 0, offs, lens, ext)[~m], gather(tgt, 0, offs, lens, ext)[~m])


# 5 ---------------------------------------------------------------- looping grid
def test_looping_grid(R, H, oracle):
    rng = np.random.default_rng(0x5EED0C50)
    lens = [int(x) for x in rng.integers(40, 110, 40)]
    lens[7] = 0
    offs, span = layout(rng, lens, 4)
    assert 2500 < sum(lens) < 3500
    tgt = make_operand(rng, 'fp', 4, span, 'MPI_FLOAT')
    org = make_operand(rng, 'fp', 4, sum(lens), 'MPI_FLOAT')
    before = R.get_launch()
    assert R.set_launch(64, 2) == 0
    try:
        for op, o in ((H.MPI_SUM, org), (H.MPI_REPLACE, org), (H.MPI_NO_OP, None)):
            fetch_iov_and_check(R, H, oracle, H.MPI_FLOAT, op, offs, lens, tgt, o,
                                ('fp', 4, 'MPI_SUM'))
    finally:
        assert R.set_launch(before['block'], before['max_grid']) == 0
    assert R.get_launch() == before


# 6 ----------------------------------------------------------------- table slots
def test_fetch_and_reduce_share_the_table_slots(R, H, oracle):
    """fetch-iov on stream A, reduce-iov on stream B, fetch-iov on stream A,
    back to back without synchronising, each with a run table of its own: the
    third call takes over the first call's slot only after its kernel is done"""
    rng = np.random.default_rng(0x5EED0C60)
    cases = []
    for nseg in (30000, 20000, 10000):
        lens = [int(x) for x in rng.integers(1, 5, nseg)]
        offs, span = layout(rng, lens, 8, gap=(0, 3))
        cases.append(Case(R, H, H.MPI_DOUBLE, H.MPI_SUM, offs, lens,
                          make_operand(rng, 'fp', 8, span, 'MPI_DOUBLE'),
                          make_operand(rng, 'fp', 8, sum(lens), 'MPI_DOUBLE')))
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    assert cases[0].fetch(a) == 0
    assert cases[1].reduce(b) == 0
    assert cases[2].fetch(a) == 0
    torch.cuda.synchronize()
    # the twins of the fetches and the fetch of the middle case, for check()
    assert cases[0].reduce() == 0 and cases[2].reduce() == 0 and cases[1].fetch() == 0
    torch.cuda.synchronize()
    for c in cases:
        c.check(oracle, ('fp', 8, 'MPI_SUM'))


# 7 -------------------------------------------------------------------- every pair
@pytest.mark.parametrize('dtname,opname,kind,size', SWEEP,
                         ids=['%s-%s' % (s[0], s[1]) for s in SWEEP])
def test_every_pair(R, H, oracle, dtname, opname, kind, size):
    dt, op = getattr(H, dtname), getattr(H, opname)
    ext = R.datatype_extent(dt)
    lens = [1, 64, 17, 0, 68]
    rng = np.random.default_rng((0x5EED0C70 * 31 + dt * 7 + op) & 0xffffffff)
    offs, span = layout(rng, lens, ext)
    tgt, org = operands(H, rng, dtname, kind, size, span, sum(lens))
    fetch_iov_and_check(R, H, oracle, dt, op, offs, lens, tgt, org, (kind, size, opname),
                        ooff=ext)


# 8 ------------------------------------------------- errors, buffers on the device
def test_refused_calls_touch_nothing(R, H):
    rng = np.random.default_rng(0x5EED0C80)
    raw = [rng.integers(0, 256, 4096, dtype=np.uint8) for _ in range(3)]
    O, Z, T = (Placed(x) for x in raw)
    offs, cnts = [0, 1024], [16, 16]            # two fp64 runs, a gap of 896 bytes between
    torch.cuda.synchronize()

    def call(o, z, t, offs=offs, cnts=cnts, dt=H.MPI_DOUBLE, op=H.MPI_SUM):
        return R.get_accumulate_local_iov(o, z, t, offs, cnts, dt, op)
    # the result inside the gap of the target's bounding range
    assert call(O.v, T.v[256:], T.v) == H.MPI_ERR_BUFFER
    assert call(T.v[256:], Z.v, T.v) == H.MPI_ERR_BUFFER
    assert call(O.v, O.v[255:], T.v) == H.MPI_ERR_BUFFER                    # origin / result
    assert call(O.v, Z.v, T.v, offs=[0, 1026]) == H.MPI_ERR_ARG             # misaligned residue
    assert call(O.v, Z.v, T.v, dt=H.MPI_BYTE, op=H.MPIX_EQUAL) == H.MPI_ERR_OP
    assert call(O.v, Z.v, T.v, dt=H.MPIX_BFLOAT16, op=H.MPI_MAX) == H.MPI_ERR_TYPE
    assert R.get_accumulate_local_iovec(O.v, Z.v, T.v, [0], [12], H.MPI_DOUBLE,
                                        H.MPI_SUM) == H.MPI_ERR_ARG
    host = np.zeros(512, np.float64)
    assert call(host, Z.v, T.v) == H.MPI_ERR_BUFFER                         # pageable operand
    torch.cuda.synchronize()
    for p, x in zip((O, Z, T), raw):
        assert np.array_equal(p.bytes(), x) and p.guards_intact()
