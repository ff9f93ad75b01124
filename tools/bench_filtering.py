"""The 2-D grid filtering experiment (filtering.py) on the real 30 x 30 grid (tests/golden/raw/TwoDGrid30.mat, recfield = 5:
323,220 mask entries, S = 11), node-level GNNML3 (models.filtering_gnnml3), Adam 1e-3, ntask 0 .. 2:

    epoch     one train step on graph 0 (dist.TrainStep + OneLaunchAdam) and eval forwards on graphs 1 and 2, every metric from the
              device `stats` sums.  Timed eagerly on the SPARSE road (CSR kernels) and on the DENSE road (csrc/gml_dense_big.hip),
              alternating epoch by epoch in one process, then the dense road as ONE captured graph per epoch (no host read per epoch).
    layers    one ML3 layer 48 -> 32 + 16 forward + backward on the same grid at recfield 2, 3, 4, 5 (mask fill 1.4 % .. 39.9 %) on
              both roads, alternating: where the dense road starts to win (models.DENSE_BIG_MIN_FILL is set from these rows).
    r2        R^2 (train / test / val) per task after --epochs captured epochs: recorded, not asserted.

One JSON line per row; --out (default profiles/filtering_twodgrid.json) writes all of it as one JSON object.

    python tools/bench_filtering.py [--epochs 200] [--iters 30] [--out profiles/filtering_twodgrid.json]
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


def _batches(recfield, dev):
    from gnn_matlang_amd import SpectralDesign, collate, readers
    recs = readers.design_twodgrid(readers.load_twodgrid(GRID), SpectralDesign(recfield=recfield, dv=10, nfreq=10))
    return [collate([r], node_fields=('y', 'mask')).to(dev) for r in recs]


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


class _Epoch(object):
    """one epoch of filtering.py:310-357 on a road: train step on graph 0, eval forwards on graphs 1 and 2; stats [3, 4] on the device"""

    def __init__(self, batches, ntask, road, dev, seed=0):
        from gnn_matlang_amd import models
        from gnn_matlang_amd.dist import TrainStep
        from gnn_matlang_amd.optim import OneLaunchAdam
        torch.manual_seed(seed)
        self.m = models.filtering_gnnml3(1, int(batches[0].edge_attr2.size(1))).to(dev)
        self.stats = torch.zeros(3, 4, device=dev)
        self.batches, self.ntask, self.road = batches, ntask, road
        self.ts = TrainStep(self.m, lambda mod, d: models.filtering_step_loss(mod, d, ntask, self.stats[0], _road=road),
                            OneLaunchAdam(self.m.parameters(), lr=1e-3))
        self.models = models

    def evals(self):
        with torch.no_grad():
            for k in (1, 2):
                self.models.filtering_step_loss(self.m, self.batches[k], self.ntask, self.stats[k], _road=self.road)

    def eager(self):
        self.ts.step(self.batches[0])
        self.evals()

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
        sp, de = _Epoch(batches, ntask, 'sparse', dev), _Epoch(batches, ntask, 'dense', dev)
        for _ in range(3):
            sp.eager()
            de.eager()
        torch.cuda.synchronize()
        ts, td = [], []
        for _ in range(iters):                                 # alternating: both roads see the same clocks
            ts.append(_timed(sp.eager))
            td.append(_timed(de.eager))
        cap = _Epoch(batches, ntask, 'dense', dev)
        replay = cap.capture()                                 # (three warm-up epochs have trained)
        hist = torch.zeros(epochs, 3, 4, device=dev)
        tc = []
        for e in range(epochs):
            tc.append(_timed(replay))
            hist[e].copy_(cap.stats)                           # device copy: nothing is read per epoch
        torch.cuda.synchronize()
        h = hist.cpu()
        r2 = [float(models.r2_from_stats(h[-1, k])) for k in range(3)]
        row = dict(row='epoch', task=name, ntask=ntask, ms_sparse_eager=statistics.median(ts), ms_dense_eager=statistics.median(td),
                   ms_dense_captured=statistics.median(tc), epochs=epochs + 3, loss_first=float(h[0, 0, 0]), loss_last=float(h[-1, 0, 0]),
                   r2_train=r2[0], r2_test=r2[1], r2_val=r2[2])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def _layers(dev, iters):
    """one ML3 layer 48 -> 32 + 16, forward + backward (d x, d W, d b), on the grid's mask at recfield 2 .. 5, both roads"""
    from gnn_matlang_amd import models
    rows = []
    for recfield in (2, 3, 4, 5):
        data = _batches(recfield, dev)[0]
        N, E, S = int(data.x.size(0)), int(data.edge_index2.size(1)), int(data.edge_attr2.size(1))
        torch.manual_seed(1)
        m = models.GNNML3(48, S, 32, 16, 1, learnedge=False, pool=None, head='node').to(dev)
        data.x = torch.randn(N, 48, device=dev, requires_grad=True)
        g = torch.randn(N, 48, device=dev)

        def run(road):
            m.zero_grad(set_to_none=True)
            data.x.grad = None
            m(data, _features=True, _road=road).backward(g)
        for _ in range(3):
            run('sparse')
            run('dense')
        torch.cuda.synchronize()
        ts, td = [], []
        for _ in range(iters):
            ts.append(_timed(lambda: run('sparse')))
            td.append(_timed(lambda: run('dense')))
        row = dict(row='layer', recfield=recfield, N=N, E=E, S=S, fill=E / float(N * N), ms_sparse=statistics.median(ts),
                   ms_dense=statistics.median(td))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=200)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'filtering_twodgrid.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    batches = _batches(5, dev)
    N, E = int(batches[0].x.size(0)), int(batches[0].edge_index2.size(1))
    out = dict(device=torch.cuda.get_device_name(0), graph=dict(N=N, E=E, S=int(batches[0].edge_attr2.size(1)), fill=E / float(N * N)),
               layers=_layers(dev, a.iters), epochs=_epochs(batches, dev, a.iters, a.epochs))
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
