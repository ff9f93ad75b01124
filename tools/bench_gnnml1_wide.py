"""Forward + backward of ONE GNNML1 block at the wide input widths of counting.py / freqclass.py (96), ptc.py (98, tanh factors) and
proteins.py (144): the fused kernels (csrc/gml_gnnml1_wide.hip) against the composition (library Linears + one S = 1 SpectConv +
elementwise ops -- what GML_NO_GNNML1_FUSED=1 selects), both roads in ONE process, alternating, timed with device events; the
median per road.  Sizes: each script's own batch, and one large batch of >= 500 k rows.

    python tools/bench_gnnml1_wide.py [--rounds 6] [--iters 100] [--out profiles/gnnml1_wide.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_matlang_amd import collate, models, synthetic            # noqa: E402
from gnn_matlang_amd import functional as Fn                       # noqa: E402
from gnn_matlang_amd.graph import GraphCSR                         # noqa: E402

# name -> (input width, (n1, n2, n3), form, graphs of the script's batch, generator arguments of its graphs)
SHAPES = dict(counting=(96, (32, 32, 32), 'product', 64, dict(nmin=10, nmax=36, p=0.3)),           # counting.py:395: 64 graphs of ~23 nodes
              freqclass=(96, (32, 32, 32), 'product', 64, dict(nmin=200, nmax=200, p=0.02)),       # freqclass.py: 64 graphs of 200 nodes
              ptc=(98, (32, 64, 2), 'tanh_factors', 60, dict(nmin=10, nmax=50, p=0.07)),           # ptc.py:398: 60 graphs of ~30 nodes
              proteins=(144, (64, 64, 16), 'factors', 180, dict(nmin=10, nmax=68, p=0.095)))       # proteins.py:310: 180 graphs of ~39 nodes


def graph(kw, ngraphs, min_rows, dev):
    """(edge_index [2, E] on dev, N): `ngraphs` random graphs, tiled until there are at least min_rows nodes"""
    b = collate([dict(x=x, edge_index=ei, y=y) for x, ei, y in synthetic.make_graphs('counting', ngraphs, seed=7, **kw)])
    ei, n = b.edge_index.to(dev), int(b.x.size(0))
    reps = max(1, -(-min_rows // n))
    if reps > 1:
        ei = torch.cat([ei + r * n for r in range(reps)], 1)
    return ei.contiguous(), n * reps


def measure(name, big, rounds, iters, dev):
    fin, widths, form, ngraphs, kw = SHAPES[name]
    ei, N = graph(kw, ngraphs, 500000 if big else 0, dev)
    csr = GraphCSR.from_edge_index(ei, N)
    torch.manual_seed(0)
    m = models.GNNML1Blocks(fin, widths, 1, form=form, pool='add', head='log_softmax', nclass=2).to(dev)
    x = torch.randn(N, fin, device=dev, requires_grad=True)
    ones = torch.ones(csr.E, 1, device=dev)
    gout = torch.randn(N, sum(widths), device=dev)
    os.environ.pop('GML_NO_GNNML1_FUSED', None)
    if not Fn.gnnml1_block_supported(x, fin, widths[0], widths[1], widths[2], models.GNNML1Blocks._MODES[form]):
        sys.exit('%s: the library does not serve this block shape' % name)

    def run():
        for q in m.parameters():
            q.grad = None
        x.grad = None
        m._block(1, x, csr, ones).backward(gout)

    ms = dict(fused=[], composition=[])
    for rnd in range(rounds + 1):                                  # round 0: the warm-up of both roads
        for road in ('fused', 'composition'):
            if road == 'composition':
                os.environ['GML_NO_GNNML1_FUSED'] = '1'
            else:
                os.environ.pop('GML_NO_GNNML1_FUSED', None)
            run()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
            ev[0].record()
            for i in range(iters):
                run()
                ev[i + 1].record()
            torch.cuda.synchronize()
            if rnd:
                ms[road] += [ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]
    os.environ.pop('GML_NO_GNNML1_FUSED', None)
    f, c = statistics.median(ms['fused']), statistics.median(ms['composition'])
    q = lambda v: [round(statistics.quantiles(v, n=10)[i], 4) for i in (0, 8)]
    return dict(shape=name, size='large' if big else 'script batch', rows=N, edges=int(csr.E), fin=fin, widths=list(widths), form=form,
                fused_ms=round(f, 4), composition_ms=round(c, 4), speedup=round(c / f, 2), fused_p10_p90=q(ms['fused']),
                composition_p10_p90=q(ms['composition']), samples=len(ms['fused']))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_gnnml1_wide.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    res = []
    measure(next(iter(SHAPES)), False, 1, a.iters, dev)           # discarded: clocks, code objects and the allocator settle here
    for big in (False, True):
        for name in SHAPES:
            res.append(measure(name, big, a.rounds, a.iters, dev))
            print(json.dumps(res[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/bench_gnnml1_wide.py', what='one GNNML1 block forward + backward, ms (median of rounds x iters '
                           'device-event intervals per road, roads alternating in one process)', rounds=a.rounds, iters=a.iters,
                           results=res), f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
