"""The collective schedules' index arithmetic, without a GPU
and without the library: tests/c/coll_sched_check.cpp built with g++ against
mpich_amd/csrc/coll_sched.h alone, as built and with AddressSanitizer +
UBSan (a program of its own; nothing is loaded into Python).

The walk: P = 1..64, every rank the fold keeps, random ragged counts with
zeros -- halve() against rs_recursive_halving's decreasing-mask loop and
allreduce_rsag's increasing-mask loop (width pof2 / (2 mask)), regrow()
against the allgather's reverse, each restated index for index in the program:
the send / receive block ranges and counts of every step, the final window
(block newrank; bitrev(newrank) for the increasing form; all blocks after the
reverse), and a step's two partners mirroring each other.  Fold for both
parities (real(newrank_of(r)) == r, pof2 survivors, the dropped rank's partner
survives, folded counts against the old loop and summing to the total).
Blocks: the even and ring splits tile [0, count) for count 0 .. 4 P + 3, range()
equals the sum of cnts.  Multipath parts and chunks tile [0, D) from
parts (parts - 1) up and at 1, 2 and 8 chunks per part; every relay mask pair
{a, a ^ m} used once.  Pipelined chunks tile every block.  rs_workspace
against the table of the old switch.  tree_slot_source: P = 2..16, every
source once per rank, absent slots only with a fold -- and the lists of
tests/golden/coll_tree_slots.json, which tests/golden/make_coll_tree_slots.py
wrote from a restatement of the two loops as they stood in rs_pull and
allreduce_pull."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def build(tmp_path, *flags):
    exe = str(tmp_path / ('coll_sched_check' + ''.join(flags).replace('=', '_').replace(',', '_')))
    subprocess.run(['g++', '-O2', '-g', '-std=c++17', '-Wall', '-Werror', *flags,
                    '-I' + os.path.join(ROOT, 'mpich_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), '-o', exe,
                    os.path.join(ROOT, 'tests', 'c', 'coll_sched_check.cpp')], check=True)
    return exe


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp('coll_sched'))


def run(exe, mode, stdin=None, env=None):
    p = subprocess.run([exe, mode], input=stdin, capture_output=True, text=True, timeout=300,
                       env=env)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    return p


def test_walk_fold_blocks_cuts(exe):
    p = run(exe, 'props')
    assert 'coll_sched props: ok' in p.stdout, p.stdout
    # P = 1..64: the sum over P of pof2 new ranks x 3 walks x log2(pof2) steps
    # (12 + 96 + 576 + 3072 + 15360 + 1152)
    assert 'walk steps: 20268' in p.stdout, p.stdout


def test_props_asan_ubsan(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS='halt_on_error=1:exitcode=66',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1:exitcode=66')
    p = run(build(tmp_path, '-fsanitize=address,undefined', '-fno-sanitize-recover=all'), 'props',
            env=env)
    assert 'coll_sched props: ok' in p.stdout
    assert 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, p.stderr[-4000:]


def test_tree_slots_golden(exe):
    with open(os.path.join(GOLDEN, 'coll_tree_slots.json')) as f:
        cases = json.load(f)['cases']
    assert {c[0] for c in cases} == set(range(2, 17)) and {c[2] for c in cases} == {0, 1}
    # every rank under the reversed order, every kept rank under the plain one
    for P in range(2, 17):
        p2 = 1 << (P.bit_length() - 1)
        assert sum(1 for c in cases if c[0] == P and c[2] == 1) == P
        assert sum(1 for c in cases if c[0] == P and c[2] == 0) == p2
    p = run(exe, 'slots', ''.join('%d %d %d\n' % tuple(c[:3]) for c in cases))
    got = [[int(x) for x in line.split(',')] for line in p.stdout.split()]
    assert got == [c[3] for c in cases]
    for P, rank, rev, slots in cases:
        assert sorted(s for s in slots if s >= 0) == list(range(P)), (P, rank, rev)
        assert (-1 in slots) == (P & (P - 1) != 0), (P, rank, rev)
