"""What every schedule of libmpix_coll posts and combines, rank by rank,
against tests/golden/coll_traces.json -- written by
tests/golden/make_coll_traces.py from the library as it stood before the
schedules' index arithmetic moved into mpich_amd/csrc/coll_sched.h.  No GPU and
no threads: a null transport and a recording combine on a host communicator,
one rank at a time (see the generator's docstring for the trace's form).

Reduce-scatter-block (recursive halving, pairwise, sequential pairwise,
multipath, auto; P = 1..17, 24, 31, 32; recvcount 1, 7, 1001; in place and
not; again with 4108-byte messages; multipath with two pipelined chunks per
part at P = 4), ragged reduce-scatter (P = 2, 3, 5, 6, 8, 13), allreduce (six
schedules, counts pof2, pof2 + 1, 1037, 8 pof2^2), reduce (binomial and
scatter-gather, every root at P <= 8, else {0, 1, 2 rem - 1, 2 rem, P - 1}),
scan and exscan (P = 1..9, 16, 17): the exchange groups in order with every
operation's peer, direction, buffer, offset and size, the combine calls in
order, the workspace query and last_rs / last_allreduce / fallbacks.

Every case holds the first 48 bits of the SHA-256 over its ranks' traces and
its group / operation / combine totals; the small cases named by the
generator's full() hold the ranks' whole traces, so a difference there can be
read.  `python tests/golden/make_coll_traces.py --ranks CASE` prints a case's
per-rank digests and counts, to find the rank that moved."""
import hashlib
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def _generator():
    spec = importlib.util.spec_from_file_location(
        'make_coll_traces', os.path.join(GOLDEN, 'make_coll_traces.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def traced():
    """(generator, fixture, {case id: (entry, per-rank traces)}) -- every case run once"""
    gen = _generator()
    with open(os.path.join(GOLDEN, 'coll_traces.json')) as f:
        gold = json.load(f)
    tr = gen.Tracer(ROOT)
    got = {}
    for case in gen.cases():
        got[gen.case_id(case)] = gen.run_case(tr, case)
    return gen, gold, got


def test_every_case_of_the_fixture_runs(traced):
    gen, gold, got = traced
    ids = [gen.case_id(c) for c in gen.cases()]
    assert len(ids) == len(set(ids)) == len(got) == len(gold['digests']) >= 2600
    assert set(gold['full']) <= set(ids) and len(gold['full']) >= 40
    assert os.path.getsize(os.path.join(GOLDEN, 'coll_traces.json')) <= \
        os.path.getsize(os.path.join(GOLDEN, 'host_routes.json'))


def test_digests(traced):
    gen, gold, got = traced
    bad = []
    for cid, want in zip((gen.case_id(c) for c in gen.cases()), gold['digests']):
        have = got[cid][0]
        if have != want:
            moved = ['%s %s -> %s' % (n, a, b) for n, a, b in
                     zip(('groups', 'ops', 'combines'), want.split(':')[1:], have.split(':')[1:])
                     if a != b]
            bad.append('%s: %s' % (cid, ', '.join(moved) or 'same counts, other content'))
    assert not bad, '%d cases moved, first: %s' % (len(bad), bad[:8])


def test_whole_traces(traced):
    gen, gold, got = traced
    for cid, want in gold['full'].items():
        have = got[cid][1]
        assert len(have) == len(want), cid
        for rank, (w, h) in enumerate(zip(want, have)):
            names = ('workspace bytes', 'exchange groups', 'combine calls', 'state')
            for name, a, b in zip(names, w, h):
                assert a == b, '%s rank %d: %s differ' % (cid, rank, name)
            assert hashlib.sha256(gen.canon(w)).digest() == hashlib.sha256(gen.canon(h)).digest()
