"""What the packet launchers decide before they launch (DESIGN.md §7 "Launch
plans"), without a GPU and without the library: tests/c/launch_plan_check.cpp
built with g++ against mpich_amd/csrc/redop_launch.h alone.

replay: every case of tests/golden/launch_plans.json (tests/golden/
make_launch_plans.py, a restatement of launch_contig, launch_multi,
launch_tree, launch_vector, launch_getacc and launch_batch as they stood in
redop_kernels.h) gives the same form, completion-word flag, grid, block, LDS
bytes, `pres` and split, and every batch the same steps; the fixture holds
every value of the form enum and both batch branches no GPU test can reach (a
flush before a segment that would pass max_blocks, a segment with more tiles
than one grid holds).  props: over units x phases x counts 0 .. 4 E block the
split adds up, its head is shorter than a packet, its tail shorter than E, its
packets start on a 16-byte boundary and the grid covers them; over 2,400 random
batches of 64 segments blk0 ascends from 0 in every launch, no launch passes
max_blocks, and every slot's split is the single call's.  The same program
once more under AddressSanitizer and UndefinedBehaviorSanitizer (a program of
its own; nothing is loaded into Python)."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mpich_amd', 'csrc')
FACTS = ('unroll', 'unroll32', 'block32', 'vblock', 'signal_max_grid', 'multi_lds')


def build(tmp_path, *flags):
    exe = str(tmp_path / 'launch_plan_check')
    subprocess.run(['g++', '-O2', '-g', '-std=c++17', '-Wall', *flags, '-I' + CSRC, '-o', exe,
                    os.path.join(ROOT, 'tests', 'c', 'launch_plan_check.cpp')], check=True)
    return exe


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp('launch_plan'))


@pytest.fixture(scope='module')
def gold():
    with open(os.path.join(ROOT, 'tests', 'golden', 'launch_plans.json')) as f:
        return json.load(f)


def flat(args):
    """a case's arguments as the check's line: a list is its length, then its items"""
    out = []
    for a in args:
        if isinstance(a, list):
            if a and isinstance(a[0], list):
                out += [len(a)] + [x for s in a for x in s]
            else:
                out += [len(a)] + a
        else:
            out.append(a)
    return out


def line(case):
    kind = case[0]
    if kind == 'batch':
        unit, segs, block, is_split = case[1:5]
        return 'batch ' + ' '.join(map(str, flat([unit, block, is_split, segs])))
    if kind == 'multi':
        unit, ins, ao, count, block, mg = case[1:7]
        return 'multi ' + ' '.join(map(str, flat([unit, ao, count, block, mg, ins])))
    if kind == 'tree':
        unit, ins, ao, count, mg, is_split = case[1:7]
        return 'tree ' + ' '.join(map(str, flat([unit, ao, count, mg, is_split, ins])))
    return kind + ' ' + ' '.join(map(str, case[1:-10]))


def want(case):
    if case[0] == 'batch':
        return ' '.join(case[-1])
    return ' '.join(map(str, case[-10:]))


def replay(exe, gold, env=None):
    text = 'facts ' + ' '.join(str(gold['facts'][k]) for k in FACTS) + '\n'
    text += ''.join(line(c) + '\n' for c in gold['cases'])
    p = subprocess.run([exe, 'replay'], input=text, capture_output=True, text=True, timeout=300,
                       env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = p.stdout.split('\n')[:-1]
    assert len(got) == len(gold['cases'])
    bad = [(c[:-1], want(c), g) for c, g in zip(gold['cases'], got) if want(c) != g]
    assert not bad, bad[:5]
    return p


def forms_of_header():
    with open(os.path.join(CSRC, 'redop_launch.h')) as f:
        body = re.search(r'enum class Form[^{]*\{(.*?)\};', f.read(), re.S).group(1)
    return set(re.findall(r'^\s*(\w+),', body, re.M))


def test_fixture_holds_every_form_and_batch_branch(gold):
    cases = gold['cases']
    golden = os.path.join(ROOT, 'tests', 'golden')
    assert os.path.getsize(os.path.join(golden, 'launch_plans.json')) <= os.path.getsize(
        os.path.join(golden, 'host_routes.json'))
    by_kind = {}
    for c in cases:
        if c[0] != 'batch':
            by_kind.setdefault(c[0], set()).add(c[-10])
    assert by_kind == {
        'contig': {'PacketsAin', 'PacketsUin', 'Elem', 'Packets32'},
        'multi': {'PacketsAin', 'Elem'},
        'tree': {'Tree2x2', 'Tree4x2', 'Tree8x1', 'Tree16x1', 'TreeElem', 'TreePair32'},
        'vector': {'VectorS2', 'Vector1', 'Vector', 'PacketsAin', 'PacketsUin', 'Packets32'},
        'getacc': {'GetaccAligned', 'GetaccUnaligned', 'GetaccElem'},
    }
    forms = set().union(*by_kind.values())
    assert forms == forms_of_header() and len(forms) == 16
    # the completion word, stored by the kernel and not
    assert {(c[7], c[8], c[-9]) for c in cases if c[0] == 'contig' and c[-8] in (1, 64, 65)} >= {
        (1, 1, 1), (1, 0, 1), (1, 0, 0), (0, 0, 0)}
    # the LDS cap, on and dropped at 64 KiB
    assert {c[-6] for c in cases if c[0] == 'multi'} == {0, gold['facts']['multi_lds']}
    for wide in (False, True):
        mid_flush = oversize = full = head_only = False
        for c in (c for c in cases if c[0] == 'batch' and (c[1] > 16) == wide and not c[4]):
            unit, segs, block = c[1:4]
            steps = c[-1]
            for a, b in zip(steps, steps[1:]):
                mid_flush |= a[0] == 'F' and b[0] == 'S'
            for s in steps:
                if s[0] == 'O':
                    ai, ao, count = segs[int(s[1:])]
                    grid = 16 if wide else unit
                    oversize |= ai % grid == 0 and ao % grid == 0
                if s[0] == 'S':
                    f = [int(x) for x in s[1:].split(',')]
                    full |= f[1] == 63
                    head_only |= f[4] == 0
        assert mid_flush and oversize and full and (head_only or wide), (wide, mid_flush, oversize,
                                                                         full, head_only)
    # a split combiner: every segment a call of its own
    assert any(c[0] == 'batch' and c[4] and all(s[0] == 'O' for s in c[-1]) for c in cases)


def test_replay(exe, gold):
    replay(exe, gold)


def test_properties(exe):
    p = subprocess.run([exe, 'props'], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and 'launch plan props: ok' in p.stdout, p.stdout[-4000:] + p.stderr
    assert 'batches: 2400' in p.stdout, p.stdout


def test_sanitized(tmp_path, gold):
    exe = build(tmp_path, '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined')
    env = dict(os.environ, ASAN_OPTIONS='halt_on_error=1:exitcode=66',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1:exitcode=66')
    p = replay(exe, gold, env)
    assert 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, p.stderr[-4000:]
    p = subprocess.run([exe, 'props'], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and 'launch plan props: ok' in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
    assert 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, p.stderr[-4000:]
