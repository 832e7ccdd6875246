"""The host-resident operands' pure host logic, without a
GPU and without the library: tests/c/hostpath_check.cpp built with g++
against mpich_amd/csrc/redop_hostpath.h alone.

wave_chunks: for chunk in {1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 1000, 16384,
2^24 + 3}, every count in 1 .. 40 x min(chunk, 64) and 300 random counts
below 200 x chunk, the chunks tile [0, count) in order, none is empty and none
exceeds `chunk` (a chunk must fit a ring half); the lists of (165, 16),
(33, 16), (5, 16) and of tests/golden/wave_chunks.json, which
tests/golden/make_wave_chunks.py wrote from a restatement of the loop as it
stood in `waved`.  slice: W = 1 .. 16 workers, the slices disjoint, in order,
covering [0, bytes), every non-empty one starting on a 4 KiB boundary.
parse_cpulist.  SpinBarrier, run_workers and FirstError: 1, 2 and 8 workers
over 2,000 steps, as built and under ThreadSanitizer (a program of its own;
nothing is loaded into Python).  host_route: every case of
tests/golden/host_routes.json (tests/golden/make_host_routes.py, a
restatement of the if-chain as it stood in MPIX_Reduce_local), each form that
can answer -1 taken to do so; the fixture holds every route and every
fallback edge."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def build(tmp_path, *flags):
    exe = str(tmp_path / ('hostpath_check' + ''.join(flags).replace('=', '_')))
    subprocess.run(['g++', '-O2', '-g', '-std=c++17', '-Wall', '-pthread', *flags,
                    '-I' + os.path.join(ROOT, 'mpich_amd', 'csrc'), '-o', exe,
                    os.path.join(ROOT, 'tests', 'c', 'hostpath_check.cpp')], check=True)
    return exe


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp('hostpath'))


def run(exe, mode, stdin=None, env=None):
    p = subprocess.run([exe, mode], input=stdin, capture_output=True, text=True, timeout=300,
                       env=env)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    return p


def test_chunks_slices_cpulist(exe):
    p = run(exe, 'props')
    assert 'hostpath props: ok' in p.stdout, p.stdout
    assert 'wave_chunks cases: 14900' in p.stdout, p.stdout


def test_wave_chunks_golden(exe):
    with open(os.path.join(GOLDEN, 'wave_chunks.json')) as f:
        cases = json.load(f)['cases']
    assert len(cases) >= 50
    want = {(165, 16): [2, 4, 8] + [16] * 8 + [8, 4, 11], (33, 16): [2, 4, 8, 8, 4, 7],
            (5, 16): [2, 3]}
    for count, chunk, sizes in cases:
        assert want.get((count, chunk), sizes) == sizes
    assert set(want) <= {(c[0], c[1]) for c in cases}
    p = run(exe, 'chunks', ''.join('%d %d\n' % (c[0], c[1]) for c in cases))
    got = [[int(x) for x in line.split(',')] for line in p.stdout.split()]
    assert got == [c[2] for c in cases]


def test_barrier_and_workers(exe):
    assert 'hostpath workers: ok' in run(exe, 'workers').stdout


def test_barrier_and_workers_tsan(tmp_path):
    env = dict(os.environ, TSAN_OPTIONS='halt_on_error=1:exitcode=66')
    p = run(build(tmp_path, '-fsanitize=thread'), 'workers', env=env)
    assert 'hostpath workers: ok' in p.stdout
    assert 'Sanitizer' not in p.stderr, p.stderr[-4000:]


def test_host_routes(exe):
    with open(os.path.join(GOLDEN, 'host_routes.json')) as f:
        gold = json.load(f)
    cases = gold['cases']
    lines = ''.join(' '.join(str(v) for v in c[:9]) + ' %d\n' % gold['chunk'] for c in cases)
    got = run(exe, 'routes', lines).stdout.split()
    assert len(got) == len(cases)
    bad = [(c, g) for c, g in zip(cases, got) if c[9] != g]
    assert not bad, bad[:10]
    # the fixture holds every route and every fallback edge
    chains = [[s.rstrip('01') for s in c[9].split('>')] for c in cases]
    assert {s for ch in chains for s in ch} == {'PS', 'PE', 'B', 'E', 'W', 'K', 'S', 'D'}
    edges = {(a, b) for ch in chains for a, b in zip(ch, ch[1:])}
    assert edges == {('B', 'E'), ('B', 'W'), ('B', 'K'), ('B', 'S'), ('W', 'S'), ('K', 'S')}
