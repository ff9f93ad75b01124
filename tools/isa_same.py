#!/usr/bin/env python3
"""Is the device code of the conv kernels the same as at <commit>?

    python tools/isa_same.py <commit> [--forward | --edge] [--kernels] [--work DIR] [file.hip ...]

Compiles each source to gfx950 device assembly (the flags of gnn_matlang_amd/_build.py plus -S --cuda-device-only), once from
`git archive <commit>` and once from the working tree, and compares the two files after dropping the lines that contain
`__hip_cuid_` (a hash of the source text: the only thing that differs when dead code is deleted).  One line per file; exit
status 1 when any differs.  Without file arguments: every gml_bwd*_fam_*.hip and gml_spectconv_bwd.hip that both trees have, or,
with --forward, every gml_fwd*_fam*.hip and gml_spectconv.hip, or, with --edge, every gml_edge_*.hip (the ML3Layer edge branch).
--kernels compares kernel by kernel (a refactor that deletes SOME instantiations of a file): each assembly is cut at its kernel
symbols, kernels that both sides have are compared, kernels that one side alone has are listed and are no difference.
--work DIR keeps the assembly there and reuses <commit>'s side on the next call (a refactor in several steps)."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CSRC = os.path.join('gnn_matlang_amd', 'csrc')
BACKWARD = ('gml_bwd*_fam*.hip', 'gml_spectconv_bwd.hip')
FORWARD = ('gml_fwd*_fam*.hip', 'gml_spectconv.hip')
EDGE = ('gml_edge_*.hip',)


def asm(tree, src, out):
    csrc = os.path.join(tree, CSRC)
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I', csrc, '-I', os.path.join(tree, 'include'),
           '-Wno-unused-result', '-S', '--cuda-device-only', os.path.join(csrc, src), '-o', out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError('%s\n%s' % (' '.join(cmd), r.stderr))
    return [l for l in open(out) if '__hip_cuid_' not in l]


_LOCAL = re.compile(r'(\.L|\b)(BB|func_begin|func_end|tmp)\d+(?=_|\b)')
_NEXT = re.compile(r'\s*\.(protected|globl|weak|hidden|type|section\s+\.(text|AMDGPU))\b')
_LABEL = re.compile(r'([A-Za-z_$][\w$.]*):')


def kernels(lines):
    """{kernel symbol: lines} of a device assembly: label .. kernel descriptor (up to the next symbol's directives) + its metadata
    entry; the function index in local labels and comments, and the comment columns that move with it, are dropped."""
    names = set(l.split()[1] for l in lines if l.lstrip().startswith('.amdhsa_kernel '))
    out = {n: [] for n in names}
    cur, closed, meta = None, False, None
    for l in lines:
        if l.startswith('amdhsa.kernels:'):
            cur, meta = None, []
            continue
        if meta is not None:                                   # entries start with '  - .key', end at the next top-level key
            if l.startswith('  - ') or not l.startswith(' '):
                name = [m.split()[-1] for m in meta if m.strip().startswith('.name:')]
                if name and name[0] in out:
                    out[name[0]] += meta
                meta = [] if l.startswith('  - ') else None
            if meta is not None:
                meta.append(l)
            continue
        label = _LABEL.match(l)
        if label and label.group(1) in names:
            cur, closed = label.group(1), False
        elif cur and closed and _NEXT.match(l) and cur not in l:
            cur = None
        if cur:
            out[cur].append(' '.join(_LOCAL.sub(lambda m: m.group(1) + m.group(2), l).split()))
            closed = closed or l.lstrip().startswith('.end_amdhsa_kernel')
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('commit')
    ap.add_argument('--work', help='directory for the assembly files (kept; the side of <commit> is reused)')
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('--forward', action='store_true', help='default file list: the conv forward instead of the backward')
    ap.add_argument('--edge', action='store_true', help='default file list: the edge branch')
    ap.add_argument('--kernels', action='store_true', help='compare kernel by kernel; list the kernels only one side has')
    ap.add_argument('files', nargs='*')
    a = ap.parse_intermixed_args()
    rev = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', a.commit], capture_output=True, text=True, check=True).stdout.strip()
    tmp = None if a.work else tempfile.TemporaryDirectory()
    work = os.path.abspath(a.work) if a.work else tmp.name
    base = os.path.join(work, rev)
    if not os.path.isdir(os.path.join(base, CSRC)):
        os.makedirs(base, exist_ok=True)
        ar = subprocess.Popen(['git', '-C', ROOT, 'archive', rev, CSRC.replace(os.sep, '/'), 'include'], stdout=subprocess.PIPE)
        subprocess.run(['tar', '-x', '-C', base], stdin=ar.stdout, check=True)
        if ar.wait():
            raise RuntimeError('git archive %s failed' % rev)
    files = a.files or sorted(os.path.basename(f) for pat in (EDGE if a.edge else FORWARD if a.forward else BACKWARD)
                              for f in glob.glob(os.path.join(ROOT, CSRC, pat)))
    files = [os.path.basename(f) for f in files]
    gone = [f for f in files if not os.path.exists(os.path.join(base, CSRC, f))]
    files = [f for f in files if f not in gone]
    os.makedirs(os.path.join(work, 'new'), exist_ok=True)

    def one(src):
        old_s = os.path.join(base, src[:-4] + '.s')
        old = [l for l in open(old_s) if '__hip_cuid_' not in l] if os.path.exists(old_s) else asm(base, src, old_s)
        new = asm(ROOT, src, os.path.join(work, 'new', src[:-4] + '.s'))
        return src, old, new

    with ThreadPoolExecutor(a.jobs) as ex:
        res = list(ex.map(one, files))
    bad = 0
    for src, old, new in res:
        if not a.kernels:
            bad += old != new
            print('%-28s %s  (%d lines at %s, %d now)' % (src, 'same' if old == new else 'DIFFERENT', len(old), rev, len(new)))
            continue
        ko, kn = kernels(old), kernels(new)
        lists = (('DIFFERENT', sorted(k for k in set(ko) & set(kn) if ko[k] != kn[k])), ('only at ' + rev, sorted(set(ko) - set(kn))),
                 ('only now', sorted(set(kn) - set(ko))))
        bad += bool(lists[0][1])
        print('%-28s %d kernels on both sides, %d differ; %d only at %s, %d only now' %
              (src, len(set(ko) & set(kn)), len(lists[0][1]), len(lists[1][1]), rev, len(lists[2][1])))
        for tag, ks in lists:
            print(''.join('    %-14s %s\n' % (tag, k) for k in ks), end='')
    for f in gone:
        print('%-28s not at %s' % (f, rev))
    print('%d of %d files differ from %s' % (bad, len(res), rev))
    if tmp:
        tmp.cleanup()
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
