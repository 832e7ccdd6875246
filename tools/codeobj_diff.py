#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of the library, object by object.

    python tools/codeobj_diff.py BUILD_A BUILD_B [OUT.txt]

For every inst_*.o that both build directories hold (mpich_amd/csrc/build of two
checkouts): the kernel names, each kernel's metadata (VGPRs, SGPRs, LDS,
scratch, kernarg size), the sha256 of .text, and, where .text differs, every
function whose bytes differ, with its instruction count on both sides and the
instructions that differ (a sample and the mnemonic pairs).  Exit status 1 when
names or metadata differ anywhere.  Produced profiles/launch_plan_refactor_codeobj.txt.
"""
import collections
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = '/opt/rocm/lib/llvm/bin/'
META = ('vgpr_count', 'sgpr_count', 'agpr_count', 'group_segment_fixed_size',
        'private_segment_fixed_size', 'kernarg_segment_size')


def run(*cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def code_object(obj, d):
    """the gfx950 ELF bundled in host object `obj`, unbundled into directory d"""
    src = os.path.join(d, os.path.basename(obj))
    shutil.copy(obj, src)
    run(LLVM + 'llvm-objdump', '--offloading', src, cwd=d)
    dev = [f for f in os.listdir(d) if 'gfx950' in f]
    assert dev, 'no gfx950 code object in %s' % obj
    return os.path.join(d, dev[0])


def describe(obj):
    """(metadata by kernel name, .text bytes, {function: (offset, size)}, the ELF's path)"""
    d = tempfile.mkdtemp()
    elf = code_object(obj, d)
    meta = {}
    for b in run(LLVM + 'llvm-readelf', '--notes', elf).split('  - .agpr_count')[1:]:
        b = '.agpr_count' + b
        name = re.search(r'\.name:\s+(\S+)', b).group(1)
        meta[name] = tuple(int(re.search(r'\.%s:\s+(\d+)' % k, b).group(1)) for k in META)
    text = os.path.join(d, 'text.bin')
    run(LLVM + 'llvm-objcopy', '--dump-section', '.text=' + text, elf)
    with open(text, 'rb') as f:
        data = f.read()
    base = None
    for ln in run(LLVM + 'llvm-readelf', '-S', '-W', elf).splitlines():
        m = re.match(r'\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)', ln)
        if m:
            base = int(m.group(1), 16)
    funcs = {}
    for ln in run(LLVM + 'llvm-readelf', '-s', '-W', elf).splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] == 'FUNC':
            funcs[f[7]] = (int(f[1], 16) - base, int(f[2]))
    return meta, data, funcs, elf


def instructions(elf, name):
    """the instructions of one function, operands included, addresses stripped"""
    out = run(LLVM + 'llvm-objdump', '-d', '--no-show-raw-insn', '--disassemble-symbols=' + name, elf)
    ins = []
    for ln in out.splitlines():
        if ln.startswith('\t'):
            ins.append(re.sub(r'\s*//.*$', '', ln.strip()))
    return ins


def main():
    a_dir, b_dir = sys.argv[1:3]
    out = open(sys.argv[3], 'w') if len(sys.argv) > 3 else sys.stdout
    objs = sorted(f for f in os.listdir(a_dir) if f.startswith('inst_') and f.endswith('.o') and
                  os.path.exists(os.path.join(b_dir, f)))
    bad = 0
    for o in objs:
        ma, ta, fa, ea = describe(os.path.join(a_dir, o))
        mb, tb, fb, eb = describe(os.path.join(b_dir, o))
        names = sorted(ma) == sorted(mb)
        meta = names and all(ma[k] == mb[k] for k in ma)
        bad += not (names and meta)
        print('%s: %d kernels, %d functions, names %s, metadata %s' % (
            o, len(ma), len(fa), 'identical' if names else 'DIFFER',
            'identical' if meta else 'DIFFER'), file=out)
        if names and not meta:
            for k in ma:
                if ma[k] != mb[k]:
                    print('    %s %s -> %s' % (k, ma[k], mb[k]), file=out)
        sa, sb = hashlib.sha256(ta).hexdigest(), hashlib.sha256(tb).hexdigest()
        print('  .text A %d bytes sha256 %s' % (len(ta), sa), file=out)
        print('  .text B %d bytes sha256 %s%s' % (len(tb), sb, '  (identical)' if sa == sb else ''),
              file=out)
        if sa == sb:
            continue
        if sorted(fa) != sorted(fb):
            print('  function lists DIFFER', file=out)
            bad += 1
            continue
        differ = [n for n in sorted(fa) if ta[fa[n][0]:fa[n][0] + fa[n][1]] !=
                  tb[fb[n][0]:fb[n][0] + fb[n][1]]]
        print('  %d of %d functions differ' % (len(differ), len(fa)), file=out)
        if not differ:
            moved = sorted(fa, key=lambda n: fa[n][0]) != sorted(fb, key=lambda n: fb[n][0])
            print('  every function byte-identical; their order in .text %s' % (
                'differs' if moved else 'is the same'), file=out)
        kinds = collections.Counter()
        for n in differ:
            ia, ib = instructions(ea, n), instructions(eb, n)
            if len(ia) != len(ib):
                print('    %s: %d -> %d instructions' % (n, len(ia), len(ib)), file=out)
                kinds['instruction count differs'] += 1
                continue
            d = [(i, x, y) for i, (x, y) in enumerate(zip(ia, ib)) if x != y]
            pairs = sorted({'%s -> %s' % (x.split()[0], y.split()[0]) for _, x, y in d})
            kinds['; '.join(pairs)] += 1
            print('    %s: %d instructions both, %d differ (at %s): %s' % (
                n, len(ia), len(d), ','.join(str(i) for i, _, _ in d[:8]), '; '.join(pairs)),
                file=out)
            for i, x, y in d[:4]:
                print('        [%d] %s  ->  %s' % (i, x, y), file=out)
        for k, v in kinds.items():
            print('  kind: %d functions: %s' % (v, k), file=out)
    print('names and metadata %s' % ('DIFFER' if bad else 'identical in all %d objects' % len(objs)),
          file=out)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
