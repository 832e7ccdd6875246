"""The host side of the typed accumulate entries under AddressSanitizer +
UndefinedBehaviorSanitizer: tests/c/typed_host_check.cpp, a stand-alone program
linked against the sanitizer build of redop_capi.cpp
(mpich_amd/csrc/sanitize.mk), builds the packed-order table of random tables of
up to 10^5 runs -- negative offsets, two residues, shuffled order, the padded
pairs' raw iov -- compares MPIX_Iov_plan_locate with its own walk of the
merged runs, and drives the entries' device-free checks on wild pointers.
CPU only; nothing is preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mpich_amd', 'csrc')


def test_typed_host_code_under_sanitizer():
    exe = os.path.join('build', 'asan', 'typed_host_check')
    subprocess.run(['make', '-s', '-f', 'sanitize.mk', 'SAN=asan', exe], cwd=CSRC, check=True,
                   timeout=600)
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'abort_on_error=0:halt_on_error=1:detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1:print_stacktrace=1'
    p = subprocess.run([os.path.join(CSRC, exe)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-6000:])
    assert 'typed_host_check: 0 errors' in p.stdout
    assert 'Sanitizer' not in p.stderr, p.stderr[-6000:]
