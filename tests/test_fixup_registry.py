"""The registry of the split combiners' fixup-word buffers,
without a GPU and without the library: tests/c/fixup_registry_check.cpp built
with g++ against mpich_amd/csrc/redop_fixup.h alone, as it is and under
ThreadSanitizer (a program of its own; nothing is loaded into Python).

A fake device gives every stream a FIFO of kernels and event markers that
complete only when the test pops them, and fails the run when a buffer is
freed twice, while a caller holds it or while a kernel that names it is still
queued, when a kernel is enqueued on a freed buffer, or when a k_fixup32 does
not directly follow its own k_contig32 in its FIFO.

shared:     8 threads x 2,000 acquire / enqueue two / release cycles on one
            stream key: one buffer, one FIFO, 16,000 pairs in order.
perthread:  the same on the per-thread handle: a buffer and a FIFO per thread.
growth:     one thread alternates small and ever larger requests while seven
            use the same key; every lease is at least the size asked for.
finalize:   one thread calls finalize over and over while seven cycle (on the
            shared key and on keys of their own), and they go on afterwards.
prune:      10,000 keys one after another, each completed: never more than
            kFixupMaxIdle buffers live; 100 keys with work pending are kept,
            and go once it completes.
allocfail:  the Nth allocation fails, N = 1 .. 8: that acquire alone reports
            it, and after finalize every buffer was freed once.
Every scenario ends drained and finalized with no buffer, event or entry left."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ['shared', 'perthread', 'growth', 'finalize', 'prune', 'allocfail']


def build(tmp_path, *flags):
    exe = str(tmp_path / ('fixup_registry_check' + ''.join(flags).replace('=', '_')))
    subprocess.run(['g++', '-O2', '-g', '-std=c++17', '-Wall', '-pthread', *flags,
                    '-I' + os.path.join(ROOT, 'mpich_amd', 'csrc'), '-o', exe,
                    os.path.join(ROOT, 'tests', 'c', 'fixup_registry_check.cpp')], check=True)
    return exe


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp('fixup'))


@pytest.fixture(scope='module')
def exe_tsan(tmp_path_factory):
    return build(tmp_path_factory.mktemp('fixup_tsan'), '-fsanitize=thread')


def run(exe, mode, env=None):
    p = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert 'fixup registry %s: ok' % mode in p.stdout, p.stdout
    return p


@pytest.mark.parametrize('mode', MODES)
def test_registry(exe, mode):
    run(exe, mode)


@pytest.mark.parametrize('mode', MODES)
def test_registry_tsan(exe_tsan, mode):
    env = dict(os.environ, TSAN_OPTIONS='halt_on_error=1:exitcode=66')
    p = run(exe_tsan, mode, env=env)
    assert 'Sanitizer' not in p.stderr, p.stderr[-4000:]


def test_unknown_mode_fails(exe):
    assert subprocess.run([exe, 'nonesuch'], capture_output=True).returncode == 2
