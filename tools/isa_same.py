#!/usr/bin/env python3
"""Is the device code of the conv-backward kernels the same as at <commit>?

    python tools/isa_same.py <commit> [--work DIR] [file.hip ...]

Compiles each source to gfx950 device assembly (the flags of gnn_matlang_amd/_build.py plus -S --cuda-device-only), once from
`git archive <commit>` and once from the working tree, and compares the two files after dropping the lines that contain
`__hip_cuid_` (a hash of the source text: the only thing that differs when dead code is deleted).  One line per file; exit
status 1 when any differs.  Without file arguments: every gml_bwd*_fam_*.hip and gml_spectconv_bwd.hip that both trees have.
--work DIR keeps the assembly there and reuses <commit>'s side on the next call (a refactor in several steps)."""
import argparse
import glob
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CSRC = os.path.join('gnn_matlang_amd', 'csrc')


def asm(tree, src, out):
    csrc = os.path.join(tree, CSRC)
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I', csrc, '-I', os.path.join(tree, 'include'),
           '-Wno-unused-result', '-S', '--cuda-device-only', os.path.join(csrc, src), '-o', out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError('%s\n%s' % (' '.join(cmd), r.stderr))
    return [l for l in open(out) if '__hip_cuid_' not in l]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('commit')
    ap.add_argument('--work', help='directory for the assembly files (kept; the side of <commit> is reused)')
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('files', nargs='*')
    a = ap.parse_args()
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
    files = a.files or sorted(os.path.basename(f) for pat in ('gml_bwd*_fam*.hip', 'gml_spectconv_bwd.hip')
                              for f in glob.glob(os.path.join(ROOT, CSRC, pat)))
    files = [os.path.basename(f) for f in files]
    gone = [f for f in files if not os.path.exists(os.path.join(base, CSRC, f))]
    files = [f for f in files if f not in gone]
    os.makedirs(os.path.join(work, 'new'), exist_ok=True)

    def one(src):
        old_s = os.path.join(base, src[:-4] + '.s')
        old = [l for l in open(old_s) if '__hip_cuid_' not in l] if os.path.exists(old_s) else asm(base, src, old_s)
        new = asm(ROOT, src, os.path.join(work, 'new', src[:-4] + '.s'))
        return src, old == new, len(old), len(new)

    with ThreadPoolExecutor(a.jobs) as ex:
        res = list(ex.map(one, files))
    for src, same, n_old, n_new in res:
        print('%-28s %s  (%d lines at %s, %d now)' % (src, 'same' if same else 'DIFFERENT', n_old, rev, n_new))
    for f in gone:
        print('%-28s not at %s' % (f, rev))
    bad = sum(not same for _, same, _, _ in res)
    print('%d of %d files differ from %s' % (bad, len(res), rev))
    if tmp:
        tmp.cleanup()
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
