"""The filtering GNNML1 (filtering.py:200-250, models.filtering_gnnml1: three blocks relu(a) + relu(c) + relu(f2 f3), 32 wide, node
head) on the real 30 x 30 grid (tests/golden/raw/TwoDGrid30.mat, 900 nodes, 3,480 adjacency entries), Adam 1e-3, ntask 0 .. 2:

    block     ONE block forward + backward (dx and all eight parameter gradients) at the model's two shapes, 1 -> 32 and 32 -> 32: the
              fused kernels (csrc/gml_gnnml1_act.hip, block mode 5) against the composition (library Linears + one S = 1 SpectConv +
              elementwise ops -- what GML_NO_GNNML1_FUSED=1 selects), both roads in ONE process, alternating round by round, timed
              with device events; median and 10th / 90th percentiles per road.  Sizes: the grid, and the grid tiled to >= 500 k rows.
    epoch     one train step on graph 0 (dist.TrainStep + OneLaunchAdam) and eval forwards on graphs 1 and 2, every metric from the
              device `stats` sums: eagerly on both roads (alternating), then the fused road as ONE captured graph per epoch.
    r2        R^2 (train / test / val) per task after --epochs captured epochs (+ 3 warm-up = the script's 203): recorded, not asserted.

One JSON line per row; --out (default profiles/filtering_gnnml1.json) writes all of it as one JSON object.  The GNNML3 of the same
script is measured by tools/bench_filtering.py (profiles/filtering_twodgrid.json).

    python tools/bench_filtering_gnnml1.py [--epochs 200] [--iters 30] [--rounds 6] [--out profiles/filtering_gnnml1.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = os.path.join(ROOT, 'tests', 'golden', 'raw', 'TwoDGrid30.mat')
TASKS = ('bandpass', 'lowpass', 'highpass')                    # filtering.py:301
WIDTH = 32
ENV = 'GML_NO_GNNML1_FUSED'


def _road(road):
    if road == 'composition':
        os.environ[ENV] = '1'
    else:
        os.environ.pop(ENV, None)


def _batches(dev):
    from gnn_matlang_amd import collate, readers
    return [collate([r], node_fields=('y', 'mask')).to(dev) for r in readers.load_twodgrid(GRID)]


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _quant(v):
    return [round(statistics.quantiles(v, n=10)[i], 4) for i in (0, 8)]


# ------------------------------------------------------------------------------------------------ one block
def _block(ei0, n0, fin, big, rounds, iters, dev):
    from gnn_matlang_amd import functional as Fn, models
    from gnn_matlang_amd.graph import GraphCSR
    reps = max(1, -(-500000 // n0)) if big else 1
    ei = torch.cat([ei0 + r * n0 for r in range(reps)], 1).contiguous() if reps > 1 else ei0
    N = n0 * reps
    csr = GraphCSR.from_edge_index(ei, N)
    torch.manual_seed(0)
    m = models.GNNML1Blocks(fin, (WIDTH,) * 3, 1, form='act_sum', act='relu', pool=None, head='node').to(dev)
    x = torch.randn(N, fin, device=dev, requires_grad=True)
    ones = torch.ones(csr.E, 1, device=dev)
    gout = torch.randn(N, WIDTH, device=dev)
    _road('fused')
    if not Fn.gnnml1_block_supported(x, fin, WIDTH, WIDTH, WIDTH, 5, 1):
        sys.exit('the library does not serve block mode 5 at %d -> %d' % (fin, WIDTH))

    def run():
        for q in m.parameters():
            q.grad = None
        x.grad = None
        m._block(1, x, csr, ones).backward(gout)

    ms = dict(fused=[], composition=[])
    for rnd in range(rounds + 1):                                  # round 0: the warm-up of both roads
        for road in ('fused', 'composition'):
            _road(road)
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
    _road('fused')
    f, c = statistics.median(ms['fused']), statistics.median(ms['composition'])
    fq, cq = _quant(ms['fused']), _quant(ms['composition'])
    return dict(row='block', size='tiled' if big else 'grid', rows=N, edges=int(csr.E), fin=fin, width=WIDTH, fused_ms=round(f, 4),
                composition_ms=round(c, 4), speedup=round(c / f, 2), fused_p10_p90=fq, composition_p10_p90=cq,
                fused_p90_below_composition_p10=bool(fq[1] < cq[0]), samples=len(ms['fused']))


# ------------------------------------------------------------------------------------------------ one epoch
class _Epoch(object):
    """one epoch of filtering.py:310-357: train step on graph 0, eval forwards on graphs 1 and 2; stats [3, 4] on the device"""

    def __init__(self, batches, ntask, dev, seed=0):
        from gnn_matlang_amd import models
        from gnn_matlang_amd.dist import TrainStep
        from gnn_matlang_amd.optim import OneLaunchAdam
        torch.manual_seed(seed)
        self.m = models.filtering_gnnml1(1).to(dev)
        self.stats = torch.zeros(3, 4, device=dev)
        self.batches, self.ntask, self.models = batches, ntask, models
        self.ts = TrainStep(self.m, lambda mod, d: models.filtering_step_loss(mod, d, ntask, self.stats[0]),
                            OneLaunchAdam(self.m.parameters(), lr=1e-3))

    def eager(self):
        self.ts.step(self.batches[0])
        with torch.no_grad():
            for k in (1, 2):
                self.models.filtering_step_loss(self.m, self.batches[k], self.ntask, self.stats[k])

    def capture(self):
        """-> replay(): the whole epoch as ONE graph (warm-up: three eager epochs on a side stream)"""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                self.eager()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.eager()
        return g.replay


def _epochs(batches, dev, iters, epochs):
    from gnn_matlang_amd import models
    rows = []
    for ntask, name in enumerate(TASKS):
        fu, co = _Epoch(batches, ntask, dev), _Epoch(batches, ntask, dev)
        for _ in range(3):
            _road('fused')
            fu.eager()
            _road('composition')
            co.eager()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(iters):                                 # alternating: both roads see the same clocks
            _road('fused')
            tf.append(_timed(fu.eager))
            _road('composition')
            tc.append(_timed(co.eager))
        _road('fused')
        cap = _Epoch(batches, ntask, dev)
        replay = cap.capture()                                 # (three warm-up epochs have trained)
        hist = torch.zeros(epochs, 3, 4, device=dev)
        tg = []
        for e in range(epochs):
            tg.append(_timed(replay))
            hist[e].copy_(cap.stats)                           # device copy: nothing is read per epoch
        torch.cuda.synchronize()
        h = hist.cpu()
        r2 = [float(models.r2_from_stats(h[-1, k])) for k in range(3)]
        row = dict(row='epoch', task=name, ntask=ntask, ms_fused_eager=statistics.median(tf), ms_composition_eager=statistics.median(tc),
                   ms_fused_captured=statistics.median(tg), fused_eager_p10_p90=_quant(tf), composition_eager_p10_p90=_quant(tc),
                   fused_captured_p10_p90=_quant(tg), epochs=epochs + 3, loss_first=float(h[0, 0, 0]), loss_last=float(h[-1, 0, 0]),
                   r2_train=r2[0], r2_test=r2[1], r2_val=r2[2])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--epochs', type=int, default=200)
    ap.add_argument('--iters', type=int, default=30, help='eager epochs per road; iterations per round of a block at the tiled size')
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--block-iters', type=int, default=100, help='iterations per round of a block at the grid size')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'filtering_gnnml1.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_filtering_gnnml1.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    batches = _batches(dev)
    ei0, n0 = batches[0].edge_index, int(batches[0].x.size(0))
    _block(ei0, n0, WIDTH, False, 1, a.block_iters, dev)       # discarded: the first shape a process measures reads high on both roads
    blocks = []
    for big in (False, True):
        for fin in (1, WIDTH):
            blocks.append(_block(ei0, n0, fin, big, a.rounds, a.iters if big else a.block_iters, dev))
            print(json.dumps(blocks[-1]), flush=True)
    out = dict(tool='tools/bench_filtering_gnnml1.py', device=torch.cuda.get_device_name(0), graph=dict(N=n0, E=int(ei0.size(1))),
               what='ms; blocks: median of rounds x iters device-event intervals per road, roads alternating in one process; epochs: '
                    'median of --iters eager epochs per road (alternating) and of --epochs replays of one captured graph',
               rounds=a.rounds, iters=a.iters, block_iters=a.block_iters, blocks=blocks, epochs=_epochs(batches, dev, a.iters, a.epochs))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
