"""The derived layouts' host arithmetic (DESIGN.md §16 "Run tables"), without a
GPU: mpich_amd/csrc/redop_runs.h through tests/c/runs_check.cpp, built with g++
against the header alone (nothing is linked from ROCm), and the library's plan
entries on the same cases.

fixture: every case of tests/golden/run_tables.json (tests/golden/
make_run_tables.py, a restatement of the parsing, scan, residue rule, merge,
grouping, both tile indexes and the packed-order table as they stood inline in
redop_capi.cpp) gives the same words: the parsed runs, the scan, the plan's
numbers, the merged runs, every residue group's table and tile index, the
packed-order table and the per-call entries' table; larger cases by their
SHA-256.  props: over 3,000 seeded random tables (1 to 4 residues, up to a few
thousand elements) the merged runs tile the packed order, every packed index
maps through its group's table to the byte of a plain walk and of locate(), the
tile words bracket every index's run, and over 20,000 random scans scan_runs
equals a 128-bit brute force.  Both once more under AddressSanitizer and
UndefinedBehaviorSanitizer (a program of its own; nothing is loaded into
Python).  library: MPIX_Iov_plan_create[_iovec]'s class, MPIX_Iov_plan_info,
_info_packed and MPIX_Iov_plan_locate at every index, case by case; this test
passed on the library as it was before the header, which ties the restatement
to that code."""
import ctypes
import hashlib
import json
import os
import subprocess

import pytest

from mpich_amd import handles as H
from mpich_amd import redop as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
AINT = ctypes.c_ssize_t


def build(tmp_path, *flags):
    exe = str(tmp_path / 'runs_check')
    subprocess.run(['g++', '-O2', '-g', '-std=c++17', '-Wall', *flags, '-D__HIP_PLATFORM_AMD__',
                    '-I/opt/rocm/include', '-I' + os.path.join(ROOT, 'include'),
                    '-I' + os.path.join(ROOT, 'mpich_amd', 'csrc'), '-o', exe,
                    os.path.join(ROOT, 'tests', 'c', 'runs_check.cpp')], check=True)
    return exe


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp('runs'))


@pytest.fixture(scope='module')
def cases():
    with open(os.path.join(GOLDEN, 'run_tables.json')) as f:
        return json.load(f)['cases']


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def replay(exe, cases, env=None):
    text = ''.join(' '.join(map(str, [int(c['form'] == 'iovec'), c['size'], c['ext'], c['nseg'],
                                      c['nulls'], len(c['offs'])] + c['offs'] + c['second'])) + '\n'
                   for c in cases)
    p = subprocess.run([exe, 'fixture'], input=text, capture_output=True, text=True, timeout=300,
                       env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = p.stdout.split('\n')[:-1]
    assert len(got) == len(cases)
    bad = []
    for c, g in zip(cases, got):
        if 'dump' in c:
            ok = g == c['dump']
        else:
            ok = (len(g.split()), sha(g)) == (c['words'], c['sha'])
        if not ok:
            bad.append((c['name'], c['form'], c.get('dump'), g[:2000]))
    assert not bad, bad[:3]
    return p


def test_fixture_holds_the_cases(cases):
    assert os.path.getsize(os.path.join(GOLDEN, 'run_tables.json')) < 100 * 1000
    assert {c['rc'] for c in cases} == {0, H.MPI_ERR_BUFFER, H.MPI_ERR_COUNT, H.MPI_ERR_ARG}
    assert {c['ext'] for c in cases} == {1, 2, 4, 8, 16, 32}
    assert {c['type'] for c in cases if c['size'] < c['ext']} == {
        'MPI_DOUBLE_INT', 'MPI_SHORT_INT', 'MPI_LONG_DOUBLE_INT'}
    ok = [c for c in cases if c['rc'] == 0]
    # element totals at the tile's edges, of the whole table and of one group
    assert {c['info'][0] for c in ok} >= {0, 255, 256, 257, 511, 512, 513}
    group_totals = set()
    for c in ok:
        w = c.get('dump', '').split()
        group_totals |= {int(w[i + 3]) for i, t in enumerate(w) if t == 'group'}
    assert group_totals >= {255, 256, 257, 511, 512, 513}
    assert {c['info'][2] for c in ok} >= {0, 1, 2, 3}
    assert any(c['info'][1] == 1 and c['info'][5] == 0 and c['info'][2] == 1 for c in ok)
    assert any(c['info'][3] < 0 for c in ok)
    assert any('sha' in c for c in cases) and sum('dump' in c for c in cases) >= 100
    for c in cases:
        size, ext = R.lib().MPIX_Datatype_size(H.as_c_int(getattr(H, c['type']))), \
            R.lib().MPIX_Datatype_extent(H.as_c_int(getattr(H, c['type'])))
        assert (size, ext) == (c['size'], c['ext']), c['type']


def test_replay(exe, cases):
    replay(exe, cases)


def test_properties(exe):
    p = subprocess.run([exe, 'props'], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and 'runs props: ok' in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
    assert 'tables: 3000 scans: 20000' in p.stdout, p.stdout


def test_sanitized(tmp_path, cases):
    exe = build(tmp_path, '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined')
    env = dict(os.environ, ASAN_OPTIONS='halt_on_error=1:exitcode=66',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1:exitcode=66')
    p = replay(exe, cases, env)
    assert 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, p.stderr[-4000:]
    p = subprocess.run([exe, 'props'], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and 'runs props: ok' in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
    assert 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, p.stderr[-4000:]


def test_library_on_every_case(cases):
    L = R.lib()
    for c in cases:
        arr = (AINT * max(1, len(c['offs'])))
        offs, second = arr(*c['offs']), arr(*c['second'])
        f = L.MPIX_Iov_plan_create_iovec if c['form'] == 'iovec' else L.MPIX_Iov_plan_create
        h = ctypes.c_void_p(0xdead)
        rc = f(c['nseg'], None if c['nulls'] & 1 else offs, None if c['nulls'] & 2 else second,
               H.as_c_int(getattr(H, c['type'])), ctypes.byref(h))
        assert rc == c['rc'], (c['name'], c['form'], rc)
        assert (h.value is None) == (rc != 0), c['name']
        if rc:
            continue
        v = [AINT() for _ in range(7)]
        assert L.MPIX_Iov_plan_info(h, *[ctypes.byref(x) for x in v[:6]]) == 0
        assert [x.value for x in v[:6]] == c['info'], (c['name'], c['form'])
        assert L.MPIX_Iov_plan_info_packed(h, ctypes.byref(v[6])) == 0
        assert v[6].value == c['pk_bytes'], (c['name'], c['form'])
        total = c['info'][0]
        if 'locate' in c or 'locate_sha' in c:
            got = []
            for p in range(total):
                assert L.MPIX_Iov_plan_locate(h, p, ctypes.byref(v[6])) == 0
                got.append(v[6].value)
            if 'locate' in c:
                assert got == c['locate'], (c['name'], c['form'])
            else:
                assert (len(got), sha(' '.join(map(str, got)))) == (c['located'], c['locate_sha'])
        assert L.MPIX_Iov_plan_locate(h, total, ctypes.byref(v[6])) == H.MPI_ERR_COUNT
        assert L.MPIX_Iov_plan_free(ctypes.byref(h)) == 0 and h.value is None
