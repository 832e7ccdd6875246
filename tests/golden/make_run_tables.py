#!/usr/bin/env python3
"""Writes tests/golden/run_tables.json: what the derived layouts' host code
makes of a caller's iov / iovec table, restated in Python from the code as it
stood inline in mpich_amd/csrc/redop_capi.cpp before redop_runs.h (the commit
"Typed accumulate and get-accumulate: a committed plan on every side"):
runs_from_iov, runs_from_iovec, the scan of getacc_runs / plan_build (total,
bounding range, the 2^56 caps), residues_aligned, plan_build's merge, its
packed-order table and both tile indexes, and group_runs (of the merged runs
for a plan, of the runs as parsed for the per-call entries).

A case holds its input, the error class MPIX_Iov_plan_create[_iovec] answers,
what MPIX_Iov_plan_info and _info_packed report, and `dump`: every word in the
order tests/c/runs_check.cpp prints them.  Larger cases keep the first 16 hex
digits of the dump's SHA-256 and its word count instead, and every case the
same of its MPIX_Iov_plan_locate answers (a plain walk of the input runs).

Run from the repository root: python tests/golden/make_run_tables.py"""
import hashlib
import json
import os

OK, ERR_BUFFER, ERR_COUNT, ERR_TYPE, ERR_ARG = 0, 1, 2, 3, 12
TOP = 1 << 56
# handle name -> (data bytes, extent)
TYPES = {'MPI_INT8_T': (1, 1), 'MPI_INT16_T': (2, 2), 'MPI_INT32_T': (4, 4), 'MPI_DOUBLE': (8, 8),
         'MPI_C_DOUBLE_COMPLEX': (16, 16), 'MPI_COMPLEX32': (32, 32), 'MPI_DOUBLE_INT': (12, 16),
         'MPI_SHORT_INT': (6, 8), 'MPI_LONG_DOUBLE_INT': (20, 32)}
WHOLE = 160         # words: a longer dump is kept as its hash


def runs_from_iov(nseg, offs, cnts):
    if nseg < 0:
        return ERR_COUNT, []
    if nseg > 0 and (offs is None or cnts is None):
        return ERR_BUFFER, []
    runs = []
    for s in range(nseg):
        if cnts[s] < 0:
            return ERR_COUNT, runs
        runs.append([offs[s], cnts[s]])
    return OK, runs


def runs_from_iovec(nseg, offs, lens, size, ext):
    if nseg < 0:
        return ERR_COUNT, []
    if nseg > 0 and (offs is None or lens is None):
        return ERR_BUFFER, []
    if ext == 0:
        return ERR_TYPE, []
    pairtype = size < ext
    runs, curr, target = [], 0, 0
    for i in range(nseg):
        if lens[i] < 0:
            return ERR_COUNT, runs
        if pairtype:
            if curr == 0:
                target = offs[i]
            curr += lens[i]
            if curr < size:
                continue
        else:
            target, curr = offs[i], lens[i]
        n = curr // size
        data = n * size
        runs.append([target, n])
        if pairtype:
            curr -= data
            if curr > 0:
                target = offs[i] + (lens[i] - curr)
        elif curr != data:
            return ERR_ARG, runs
    return OK, runs


def scan(runs, ext):
    cap = TOP // ext
    total = lo = hi = 0
    over = any_ = False
    for off, n in runs:
        if n == 0:
            continue
        if n > cap or total + n > cap:
            over = True
            break
        total += n
        a, b = off, off + n * ext
        if not any_ or a < lo:
            lo = a
        if not any_ or b > hi:
            hi = b
        any_ = True
    return total, lo, hi, over


def residues_aligned(runs, e):
    align = e if e < 4 else 4
    return all((off % e) % align == 0 for off, n in runs)      # Python's % is ((x % e) + e) % e


def merge(runs, e):
    out = []
    for off, n in runs:
        if n == 0:
            continue
        if out and out[-1][0] + out[-1][1] * e == off:
            out[-1][1] += n
        else:
            out.append([off, n])
    return out


def tile_index(prefix, n, total):
    ntile = (total + 255) // 256
    s, out = 0, []
    for t in range(ntile):
        while s + 1 < n and prefix[s + 1] <= t * 256:
            s += 1
        out.append(s)
    return out + [n - 1]


def group_runs(runs, e):
    """[(resid, nrun, gtotal, [seg_off n][prefix n+1][src_off n])] in order of first use"""
    resid, groups = [], []
    for k, (off, n) in enumerate(runs):
        if n == 0:
            continue
        r = off % e
        if r not in resid:
            resid.append(r)
            groups.append([])
        groups[resid.index(r)].append(k)
    src_of, src = [], 0
    for off, n in runs:
        src_of.append(src)
        src += n
    out = []
    for r, ks in zip(resid, groups):
        seg, prefix, srcs, pre = [], [], [], 0
        for k in ks:
            seg.append((runs[k][0] - r) // e)
            prefix.append(pre)
            srcs.append(src_of[k])
            pre += runs[k][1]
        out.append((r, len(ks), pre, seg + prefix + [pre] + srcs))
    return out


def flat(runs):
    return [len(runs)] + [x for r in runs for x in r]


def restate(form, size, ext, nseg, offs, second):
    """(rc, info, pk_bytes, dump words, locate answers)"""
    rc, runs = (runs_from_iovec(nseg, offs, second, size, ext) if form == 'iovec'
                else runs_from_iov(nseg, offs, second))
    w = ['parse', rc]
    if rc != OK:
        return rc, None, None, w, None
    total, lo, hi, over = scan(runs, ext)
    aligned = residues_aligned(runs, ext)
    w += ['runs'] + flat(runs) + ['scan', total, lo, hi, int(over), 'aligned', int(aligned)]
    rc = OK
    if over or total != 0:
        if not aligned:
            rc = ERR_ARG
        elif over or hi - lo >= TOP or total * ext >= TOP:
            rc = ERR_COUNT
    w += ['build', rc]
    if rc != OK:
        return rc, None, None, w, None
    merged = merge(runs, ext)
    m = len(merged)
    one_off = merged[0][0] if m == 1 else 0
    groups, tiles, pk, pk_bytes, table_bytes, tile_pos = [], [], [], 0, 0, 0
    if m > 1:
        prefix = [0]
        for off, n in merged:
            prefix.append(prefix[-1] + n)
        pk_tile = tile_index(prefix, m, total)
        pk = prefix + [off for off, n in merged] + pk_tile
        pk_bytes = (2 * m + 1) * 8 + len(pk_tile) * 4
        groups = group_runs(merged, ext)
        tiles = [tile_index(tab[n:2 * n + 1], n, gtotal) for r, n, gtotal, tab in groups]
        tile_pos = 8 * sum(len(g[3]) for g in groups)
        table_bytes = tile_pos + 4 * sum(len(t) for t in tiles)
    w += ['plan', total, m, lo, hi, one_off, table_bytes, pk_bytes, len(groups), tile_pos]
    w += ['merged'] + flat(merged)
    for (r, n, gtotal, tab), tl in zip(groups, tiles):
        w += ['group', r, n, gtotal, 'tab'] + tab + ['tile'] + tl
    if pk:
        w += ['pk'] + pk
    if total:
        for r, n, gtotal, tab in group_runs(runs, ext):
            w += ['calltab', r, n, gtotal, 'tab'] + tab
    info = [total, m, 1 if m == 1 else len(groups), lo, hi, table_bytes]
    locate = None if total > 4096 else [off + j * ext for off, n in runs for j in range(n)]
    return OK, info, pk_bytes, w, locate


def sha(words):
    return hashlib.sha256(' '.join(map(str, words)).encode()).hexdigest()[:16]


def iovec_of(runs, size, ext, how):
    """the raw iovec of element runs of a pair type {value, int}: `seg` one
    segment per member, `merged` touching members in one segment (SHORT_INT's int
    touches the next element's short, so a segment ends inside an element),
    `carry` every longer segment cut 2 bytes before its end"""
    first, loc = {12: (8, 8), 6: (2, 4), 20: (16, 16)}[size]    # the value's bytes, the int's offset
    segs = []
    for off, n in runs:
        for k in range(n):
            segs += [[off + k * ext, first], [off + k * ext + loc, size - first]]
    if how == 'merged':
        out = []
        for o, ln in segs:
            if out and out[-1][0] + out[-1][1] == o:
                out[-1][1] += ln
            else:
                out.append([o, ln])
        segs = out
    if how == 'carry':
        out = []
        for o, ln in segs:
            if ln > 2:
                out += [[o, ln - 2], [o + ln - 2, 2]]
            else:
                out.append([o, ln])
        segs = out
    return [s[0] for s in segs], [s[1] for s in segs]


def cases():
    c = []

    def add(name, typ, offs, second, form='iov', nseg=None, nulls=0):
        c.append(dict(name=name, form=form, type=typ, nseg=len(offs) if nseg is None else nseg,
                      nulls=nulls, offs=offs, second=second))

    D = 'MPI_DOUBLE'
    add('empty table', D, [], [])
    add('empty table', D, [], [], 'iovec')
    add('only zero-length runs, wild and misaligned', D, [3, -(1 << 62), (1 << 62) + 5, 64], [0] * 4)
    add('only zero-length runs, wild and misaligned', D, [3, -(1 << 62), (1 << 62) + 5], [0] * 3,
        'iovec')
    add('one run', D, [40], [5])
    add('one run', D, [40], [40], 'iovec')
    add('two runs that merge', D, [0, 32], [4, 3])
    add('two runs that merge', D, [0, 32], [32, 24], 'iovec')
    add('a zero-length run between two that merge', D, [0, 1000, 32], [4, 0, 3])
    add('all runs merge into one', D, [-16, 0, 0, 24], [2, 3, 0, 1])
    add('adjacent in memory, not consecutive in call order', D, [0, 800, 32], [4, 2, 3])
    add('adjacent in memory, reversed call order', D, [32, 0], [3, 4])
    add('negative offsets', D, [-64, -20, -8], [2, 1, 1])
    add('negative offsets', 'MPI_COMPLEX32', [-64, -60, -28], [1, 1, 2])
    add('two residue groups interleaved', D, [0, 100, 48, 140, 96], [2, 3, 1, 2, 4])
    add('three residue groups interleaved', 'MPI_C_DOUBLE_COMPLEX',
        [0, 100, 8, 48, 148, 200, 96], [1, 2, 3, 1, 2, 1, 2])
    add('three residue groups interleaved', 'MPI_C_DOUBLE_COMPLEX',
        [0, 100, 8, 48, 148], [16, 32, 48, 16, 32], 'iovec')
    for t in (255, 256, 257, 511, 512, 513):
        add('one group of %d elements' % t, D, [0, 8 * t], [t - 100, 100])
        add('a group of %d elements beside one of 3' % t, D, [0, 16 * t + 4, 8 * t], [t - 100, 3, 100])
        add('two groups, %d elements in all' % t, 'MPI_INT32_T', [0, 8 * t, 16 * t],
            [t - 130, 100, 30])
    add('300 runs of one element', D, [16 * k for k in range(300)], [1] * 300)
    add('300 runs of one element, two groups', D, [16 * k + 4 * (k % 3 == 0) for k in range(300)],
        [1] * 300)
    add('one run across five tiles', D, [-80, 0, 16000], [1, 1100, 2])
    add('one run across five tiles, alone', D, [8], [1100])
    for typ, bad in (('MPI_INT8_T', None), ('MPI_INT16_T', 1), ('MPI_INT32_T', 2), ('MPI_DOUBLE', 2),
                     ('MPI_C_DOUBLE_COMPLEX', 6), ('MPI_COMPLEX32', 9)):
        e = TYPES[typ][1]
        good = 0 if e < 8 else 4
        add('extent %d' % e, typ, [good, 10 * e + good, 20 * e], [3, 2, 1])
        add('extent %d, a residue below zero' % e, typ, [3 * e if e < 8 else e - 4, 7 * e, -e - good],
            [2, 2, 2])
        if bad is not None:
            add('extent %d, a misaligned residue' % e, typ, [0, 10 * e + bad], [3, 2])
            add('extent %d, a misaligned residue in an empty run' % e, typ, [0, 10 * e + bad],
                [3, 0])
            add('extent %d, a misaligned residue in an empty run alone' % e, typ, [10 * e + bad],
                [0])
    for typ in ('MPI_DOUBLE_INT', 'MPI_SHORT_INT', 'MPI_LONG_DOUBLE_INT'):
        size, ext = TYPES[typ]
        for how in ('seg', 'merged', 'carry'):
            o, ln = iovec_of([[0, 2], [5 * ext, 1], [6 * ext, 2], [-3 * ext, 1]], size, ext, how)
            add('%s raw iovec, %s' % (typ, how), typ, o, ln, 'iovec')
        add('%s one segment of three elements and a half' % typ, typ, [0], [3 * size + size // 2],
            'iovec')
        add('%s a segment that never completes an element' % typ, typ, [0], [size - 1], 'iovec')
    add('a length that is no multiple of the size', D, [0], [12], 'iovec')
    add('a length that is no multiple of the size, second segment', 'MPI_INT32_T', [0, 64], [8, 6],
        'iovec')
    add('a negative count', D, [0, 64], [2, -1])
    add('a negative length', D, [0, 64], [16, -8], 'iovec')
    add('a negative length in a pair type', 'MPI_DOUBLE_INT', [0, 8], [8, -4], 'iovec')
    add('negative nseg', D, [0], [8], nseg=-1)
    add('negative nseg', D, [0], [8], 'iovec', nseg=-1)
    for form in ('iov', 'iovec'):
        add('null offsets', D, [0], [8], form, nulls=1)
        add('null second array', D, [0], [8], form, nulls=2)
        add('null arrays, nseg 0', D, [], [], form, nulls=3)
    for typ in ('MPI_INT8_T', 'MPI_DOUBLE', 'MPI_COMPLEX32'):
        e = TYPES[typ][1]
        add('a run of 2^56 / ext elements', typ, [0], [TOP // e])
        add('a run above 2^56 / ext', typ, [0, 0], [1, TOP // e + 1])
        add('a run one below 2^56 / ext', typ, [0], [TOP // e - 1])
        add('a running total above 2^56 / ext', typ, [0, 0, 0], [TOP // e - 1, 1, 1])
        add('a running total of 2^56 / ext', typ, [0, 0], [TOP // (2 * e), TOP // (2 * e)])
        add('a small total whose span reaches 2^56', typ, [0, TOP - e], [1, 1])
        add('a small total whose span stays below 2^56', typ, [0, TOP - 2 * e], [1, 1])
        add('a span of 2^56 across zero', typ, [-(TOP // 2), TOP // 2 - e], [1, 1])
    add('a span past 64 bits', D, [-(1 << 62), 1 << 62], [1, 1])
    add('an empty run bounds nothing', D, [0, 1 << 62], [1, 0])
    add('over before a misaligned residue', D, [0, 2], [TOP, 1])
    add('a run above 2^56 / ext, iovec', D, [0], [TOP + 8], 'iovec')
    return c


def main():
    out = []
    for c in cases():
        size, ext = TYPES[c['type']]
        offs = None if c['nulls'] & 1 else c['offs']
        second = None if c['nulls'] & 2 else c['second']
        rc, info, pk_bytes, words, locate = restate(c['form'], size, ext, c['nseg'], offs, second)
        c.update(size=size, ext=ext, rc=rc, info=info, pk_bytes=pk_bytes)
        if len(words) <= WHOLE:
            c['dump'] = ' '.join(map(str, words))
        else:
            c.update(words=len(words), sha=sha(words))
        if locate is not None:
            if len(locate) <= 16:
                c['locate'] = locate
            else:
                c.update(located=len(locate), locate_sha=sha(locate))
        out.append(c)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'run_tables.json')
    with open(path, 'w') as f:
        f.write('{"cases": [\n' + ',\n'.join(json.dumps(c) for c in out) + '\n]}\n')
    print('%d cases, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
