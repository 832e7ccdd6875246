"""Posting traces of libmpix_coll's schedules, one rank at a time (no threads,
no GPU): what tests/golden/coll_traces.json holds and tests/test_coll_traces.py
regenerates.

A custom MPIX_XPORT_HOST communicator gets an exchange function that records
its group and returns 0 at once and a combine function that records its
arguments and does nothing.  On such a communicator no schedule waits for a
peer, so rank r of P runs to the end alone.  The caller passes its own
workspace, sized by the matching *_workspace query, so every address a
schedule hands out lies in sendbuf, recvbuf or the workspace and is written as
(`s` | `r` | `w`, offset); any other address fails the generator.

A rank's trace: [workspace bytes, exchange groups, combine calls, state] with
a group a list of [peer, is_recv, buffer, offset, bytes], a combine call
[in buffer, in offset, inout buffer, inout offset, count] and state
[last_rs, last_allreduce, fallbacks].  A case is every rank of one
(collective, algorithm, P, shape, axes); the fixture keeps per case the first
48 bits of the SHA-256 over the ranks' canonical traces and the case's group,
op and combine totals, and the ranks' whole traces for the small cases named
in FULL.

    python tests/golden/make_coll_traces.py [--tree DIR] [--out FILE]
    python tests/golden/make_coll_traces.py [--tree DIR] --ranks CASE_ID

--tree: the checkout whose built libraries are traced (default: this one).
--ranks prints the per-rank digests and counts of one case, to find the rank
that moved by running it on two builds.
"""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'coll_traces.json')

MPI_INT, MPI_SUM, EXT = 0x4c000405, 0x58000003, 4
PS = list(range(1, 18)) + [24, 31, 32]
RSB_ALGS = ['recursive_halving', 'pairwise', 'pairwise_sequential', 'recursive_halving_multipath',
            'auto']
AR_ALGS = ['reduce_scatter_allgather', 'rsag_rd_allgather', 'recursive_doubling', 'ring',
           'rsag_multipath', 'auto']
REDUCE_ALGS = {'binomial': 1, 'scatter_gather': 2}
MAXMSG = 4108
BIG_RC = 1 << 21        # P = 4 multipath: 8 MiB parts, two pipelined chunks per part


def pof2_of(n):
    p = 1
    while p * 2 <= n:
        p *= 2
    return p


def cases():
    """every case id, in the fixture's order"""
    for mm in (0, MAXMSG):
        for alg in RSB_ALGS:
            for P in PS:
                for rc in (1, 7, 1001):
                    for ip in (0, 1):
                        yield ('rsb', alg, P, rc, ip, mm)
    yield ('rsb', 'recursive_halving_multipath', 4, BIG_RC, 0, 0)
    for alg in RSB_ALGS:
        for P in (2, 3, 5, 6, 8, 13):
            for shape in ('ragged', 'one'):
                for ip in (0, 1):
                    yield ('rs', alg, P, shape, ip, 0)
    for alg in AR_ALGS:
        for P in PS:
            p2 = pof2_of(P)
            for count in (p2, p2 + 1, 1037, p2 * p2 * 8):
                for ip in (0, 1):
                    yield ('allreduce', alg, P, count, ip, 0)
    for alg in REDUCE_ALGS:
        for P in PS:
            rem = P - pof2_of(P)
            roots = range(P) if P <= 8 else sorted({0, 1, max(2 * rem - 1, 0), 2 * rem, P - 1})
            for root in roots:
                for count in (pof2_of(P), 1037):
                    yield ('reduce', alg, P, count, root, 0)
    for coll in ('scan', 'exscan'):
        for P in list(range(1, 10)) + [16, 17]:
            yield (coll, '-', P, 257, 0, 0)


# whole traces are kept for these (a failure there can be read)
def full(case):
    coll, alg, P, shape, axis, mm = case
    if P < 2 or P > 4 or mm or alg == 'auto':
        return False
    if coll == 'rsb':
        return shape == 7
    if coll == 'allreduce':
        return shape == pof2_of(P) + 1 and axis == 1
    if coll == 'reduce':
        return shape == pof2_of(P) and axis in (0, P - 1)
    return coll == 'rs' and shape == 'ragged' and axis == 1 or coll == 'scan'


def case_id(case):
    return '/'.join(str(x) for x in case)


def rs_counts(P, shape):
    if shape == 'one':
        return [0] * (P - 1) + [1009]
    counts = [(r * 797) % 2011 for r in range(P)]
    counts[1 if P > 1 else 0] = 0
    return counts


class Tracer:
    def __init__(self, tree):
        sys.path.insert(0, tree)
        from mpich_amd import ccl
        assert os.path.dirname(os.path.dirname(os.path.abspath(ccl.__file__))) == \
            os.path.abspath(tree), ccl.__file__
        self.ccl, self.L = ccl, ccl.lib()
        self.bufs = {}
        self.where = []
        self.groups, self.combines = [], []
        unpack = struct.Struct('iiQQ').iter_unpack      # MPIX_P2p_op
        string_at = ctypes.string_at

        def exchange(ctx, rank, ops, nops, stream):
            self.groups.append([(peer, is_recv) + self.loc(buf) + (n,)
                                for peer, is_recv, buf, n in unpack(string_at(ops, 24 * nops))])
            return 0

        def combine(inbuf, inout, count, dt, op, stream):
            self.combines.append(self.loc(inbuf) + self.loc(inout) + (count,))
            return 0

        self.xfn = ccl.EXCHANGE_FN(exchange)
        self.cfn = ccl.COMBINE_FN(combine)

    def loc(self, addr):
        for name, lo, hi in self.where:
            if lo <= addr < hi:
                return (name, addr - lo)
        raise AssertionError('address %#x outside sendbuf, recvbuf and workspace' % addr)

    def buf(self, name, nbytes):
        """a host buffer of at least nbytes (kept and reused), registered as `name`"""
        have = self.bufs.get(name)
        if have is None or len(have) < nbytes:
            have = self.bufs[name] = (ctypes.c_char * max(nbytes, 1 << 16))()
        a = ctypes.addressof(have)
        self.where.append((name, a, a + max(nbytes, 1)))
        return a

    def rank_trace(self, case, rank):
        coll, alg, P, shape, axis, mm = case
        L, ccl = self.L, self.ccl
        h = ctypes.c_void_p()
        rc = L.MPIX_Comm_create_custom(rank, P, ctypes.cast(self.xfn, ctypes.c_void_p), None,
                                       ccl.XPORT_HOST, ctypes.byref(h))
        assert rc == 0, rc
        try:
            assert L.MPIX_Comm_set_combine(h, ctypes.cast(self.cfn, ctypes.c_void_p)) == 0
            if mm:
                assert L.MPIX_Comm_set_max_message(h, mm) == 0
            self.where, self.groups, self.combines = [], [], []
            if coll in ('rsb', 'rs'):
                a = ccl.RSB_ALGORITHMS[alg]
                counts = [shape] * P if coll == 'rsb' else rs_counts(P, shape)
                cnts = (ctypes.c_ssize_t * P)(*counts)
                need = L.MPIX_Reduce_scatter_block_workspace(shape, MPI_INT, h, a) \
                    if coll == 'rsb' else L.MPIX_Reduce_scatter_workspace(cnts, MPI_INT, h, a)
                total = sum(counts) * EXT
                r = self.buf('r', total)
                s = None if axis else self.buf('s', total)
                w = self.buf('w', need)
                rc = L.MPIX_Reduce_scatter_block(s, r, shape, MPI_INT, MPI_SUM, h, a, w, need) \
                    if coll == 'rsb' else L.MPIX_Reduce_scatter(s, r, cnts, MPI_INT, MPI_SUM, h, a,
                                                                w, need)
            elif coll == 'allreduce':
                need = L.MPIX_Allreduce_workspace(shape, MPI_INT, h)
                r = self.buf('r', shape * EXT)
                s = None if axis else self.buf('s', shape * EXT)
                w = self.buf('w', need)
                rc = L.MPIX_Allreduce(s, r, shape, MPI_INT, MPI_SUM, h, ccl.AR_ALGORITHMS[alg], w,
                                      need)
            elif coll == 'reduce':
                need = L.MPIX_Reduce_workspace(shape, MPI_INT, axis, h)
                r = self.buf('r', shape * EXT)
                s = self.buf('s', shape * EXT)
                w = self.buf('w', need)
                rc = L.MPIX_Reduce(s, r, shape, MPI_INT, MPI_SUM, axis, h, REDUCE_ALGS[alg], w, need)
            else:
                need = L.MPIX_Scan_workspace(shape, MPI_INT, h)
                r = self.buf('r', shape * EXT)
                s = self.buf('s', shape * EXT)
                w = self.buf('w', need)
                rc = (L.MPIX_Scan if coll == 'scan' else L.MPIX_Exscan)(s, r, shape, MPI_INT,
                                                                        MPI_SUM, h, w, need)
            assert rc == 0, (case, rank, rc)
            v = [ctypes.c_int() for _ in range(5)]
            assert L.MPIX_Comm_get_state(h, *[ctypes.byref(x) for x in v]) == 0
            return [need, self.groups, self.combines, [v[1].value, v[2].value, v[4].value]]
        finally:
            L.MPIX_Comm_free(h)


def canon(trace):
    return json.dumps(trace, separators=(',', ':')).encode()


def counts_of(trace):
    return [len(trace[1]), sum(len(g) for g in trace[1]), len(trace[2])]


def run_case(tr, case):
    """(entry of the fixture, whole per-rank traces) of one case"""
    P = case[2]
    sha = hashlib.sha256()
    tot = [0, 0, 0]
    traces = []
    for rank in range(P):
        t = json.loads(canon(tr.rank_trace(case, rank)))   # tuples -> lists, as the fixture reads
        traces.append(t)
        sha.update(canon(t))
        tot = [a + b for a, b in zip(tot, counts_of(t))]
    return '%s:%d:%d:%d' % (sha.hexdigest()[:12], *tot), traces


def generate(tree):
    tr = Tracer(tree)
    digests, whole = [], {}
    for case in cases():
        entry, traces = run_case(tr, case)
        digests.append(entry)
        if full(case):
            whole[case_id(case)] = traces
    return {'format': 'digests[i] = "<sha256[:12] over the ranks\' traces>:groups:ops:combines" '
                      'of the i-th case of make_coll_traces.cases(); full = whole per-rank traces',
            'digests': digests, 'full': whole}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--ranks')
    a = ap.parse_args()
    if a.ranks:
        case = next(c for c in cases() if case_id(c) == a.ranks)
        tr = Tracer(a.tree)
        for rank in range(case[2]):
            t = json.loads(canon(tr.rank_trace(case, rank)))
            print(rank, hashlib.sha256(canon(t)).hexdigest(), *counts_of(t))
        return
    gold = generate(a.tree)
    with open(a.out, 'w') as f:
        json.dump(gold, f, separators=(',', ':'))
        f.write('\n')
    print('%d cases, %d whole, %d bytes' % (len(gold['digests']), len(gold['full']),
                                            os.path.getsize(a.out)))


if __name__ == '__main__':
    main()
