"""Forward + backward (dx and all eight parameter gradients) of ONE GNNML1 block in the sum-and-factors form of enzymes_contfeat.py
at its two shapes, (22 -> 192) and (192 -> 192) with parts 128 | 128 | 64: the fused kernels (csrc/gml_gnnml1_sum.hip) against the
composition (library Linears + one S = 1 SpectConv + elementwise ops -- what GML_NO_GNNML1_FUSED=1 selects), both roads in ONE
process, alternating, timed with device events; the median and the 10th / 90th percentiles per road.  Sizes: the script's batch (60
ENZYMES graphs of tests/golden/raw/enzymes.mat, about 2 k rows) and the same batch tiled to at least 500 k rows.

    python tools/bench_gnnml1_sum.py [--rounds 6] [--iters 100] [--out profiles/gnnml1_sum.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnn_matlang_amd import collate, models, readers                # noqa: E402
from gnn_matlang_amd import functional as Fn                        # noqa: E402
from gnn_matlang_amd.graph import GraphCSR                          # noqa: E402

WIDTHS = (128, 128, 64)
SHAPES = dict(first=22, second=192)                                 # block name -> input width


def graph(min_rows, dev):
    """(edge_index [2, E] on dev, N): the script's batch -- 60 graphs, enzymes_contfeat.py:373 --, tiled until there are min_rows nodes"""
    raw = readers.load_tu(os.path.join(ROOT, 'tests', 'golden', 'raw', 'enzymes.mat'), 'enzymes', contfeat=True)
    pick = np.random.default_rng(7).permutation(len(raw))[:60]
    b = collate([dict(x=raw[i][0], edge_index=raw[i][1], y=raw[i][2]) for i in pick])
    ei, n = b.edge_index.to(dev), int(b.x.size(0))
    reps = max(1, -(-min_rows // n))
    if reps > 1:
        ei = torch.cat([ei + r * n for r in range(reps)], 1)
    return ei.contiguous(), n * reps


def measure(name, big, rounds, iters, dev):
    fin = SHAPES[name]
    ei, N = graph(500000 if big else 0, dev)
    csr = GraphCSR.from_edge_index(ei, N)
    torch.manual_seed(0)
    m = models.GNNML1Blocks(fin, WIDTHS, 1, form='sum_factors', pool='add', head='log_softmax', nclass=6).to(dev)
    x = torch.randn(N, fin, device=dev, requires_grad=True)
    ones = torch.ones(csr.E, 1, device=dev)
    gout = torch.randn(N, WIDTHS[0] + WIDTHS[2], device=dev)
    os.environ.pop('GML_NO_GNNML1_FUSED', None)
    if not Fn.gnnml1_block_supported(x, fin, WIDTHS[0], WIDTHS[1], WIDTHS[2], 4):
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
    fq, cq = q(ms['fused']), q(ms['composition'])
    return dict(shape=name, size='large' if big else 'script batch', rows=N, edges=int(csr.E), fin=fin, widths=list(WIDTHS),
                fused_ms=round(f, 4), composition_ms=round(c, 4), speedup=round(c / f, 2), fused_p10_p90=fq, composition_p10_p90=cq,
                fused_p90_below_composition_p10=bool(fq[1] < cq[0]), samples=len(ms['fused']))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--big-iters', type=int, default=20, help='iterations per round at the large size')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_gnnml1_sum.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    res = []
    # discarded, at full length: the (22 -> 192) block read 0.26 - 0.33 / 0.76 - 0.89 ms (fused / composition) when it was the first
    # shape a process measured after one warm-up round, and 0.16 / 0.59 ms when it was measured later in the same process -- on both
    # roads alike, so it is no property of either; the cause is not established
    measure('second', False, a.rounds, a.iters, dev)
    measure('first', False, a.rounds, a.iters, dev)
    for big in (False, True):
        for name in SHAPES:
            res.append(measure(name, big, a.rounds, a.big_iters if big else a.iters, dev))
            print(json.dumps(res[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/bench_gnnml1_sum.py', what='one GNNML1 sum-and-factors block forward + backward, ms (median of '
                           'rounds x iters device-event intervals per road, roads alternating in one process)', rounds=a.rounds,
                           iters=a.iters, big_iters=a.big_iters, results=res), f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
