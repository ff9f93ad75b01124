"""The EXP classification experiment (exp_classify.py) on the real 1,200 graphs (tests/golden/raw/exp.npz, SpectralDesign(recfield=1,
dv=2, nfreq=5, adddegree=True): 2 input features, 6 supports), batch 50, Adam 1e-3, GNNML3 (models.exp_classify_gnnml3) and GNNML1
(models.exp_classify_gnnml1).  An epoch is 16 train steps over graphs [400, 1200) (shuffled) + 4 val forwards over [0, 200) + 4 test
forwards over [200, 400); every metric comes from the device `stats` sums of models.exp_classify_step_loss.

    epoch     the epoch timed three ways -- eagerly over plain batches (DeviceDataset.batch), eagerly over static batches
              (batch_assembled), and as ONE captured train step replayed per batch + ONE captured eval forward replayed per eval batch
              with `stats` read once per epoch -- each with the fused head (functional.HeadBCEFunction) and with the torch-op road
              (GML_NO_HEAD_BCE), the two alternating epoch by epoch in one process.
    curves    train / val / test loss and accuracy per epoch over --epochs captured epochs, under the default arithmetic and under
              functional.exact_products(): the experiment lives on differences of 1e-3 .. 1e-4 between the two graphs of a pair.
    large     one train step (forward + backward + Adam) on the data set tiled to >= 600,000 nodes in ONE batch: the workspace form
              of the head (more than 256 pooled rows).

Recorded, not asserted.  One JSON line per row; --out (default profiles/exp_classify.json) writes all of it as one JSON object.

    python tools/bench_exp_classify.py [--epochs 200] [--iters 20] [--out profiles/exp_classify.json]
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXP = os.path.join(ROOT, 'tests', 'golden', 'raw', 'exp.npz')
BS = 50                                                        # exp_classify.py:19-21
SPLITS = dict(val=(0, 200), test=(200, 400), train=(400, 1200))


def _dataset(dev):
    from gnn_matlang_amd import SpectralDesign, readers
    from gnn_matlang_amd.dataset import DeviceDataset
    gs = SpectralDesign(nmax=64, recfield=1, dv=2, nfreq=5, adddegree=True).design_many(readers.load_exp(EXP))   # exp_classify.py:16
    assert [len(s) for s in readers.exp_classify_splits(gs)] == [200, 200, 800]
    dd = DeviceDataset.from_graphs(gs, dev)
    dd.y = dd.y.float()
    return dd


def _model(which, dev, seed=0):
    from gnn_matlang_amd import models
    torch.manual_seed(seed)
    return {'gnnml3': models.exp_classify_gnnml3, 'gnnml1': models.exp_classify_gnnml1}[which]().to(dev).train()


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


@contextlib.contextmanager
def _head(fused):
    """the road exp_classify_step_loss takes inside the block (a captured graph keeps the road it was captured with)"""
    old = os.environ.pop('GML_NO_HEAD_BCE', None)
    if not fused:
        os.environ['GML_NO_HEAD_BCE'] = '1'
    try:
        yield
    finally:
        os.environ.pop('GML_NO_HEAD_BCE', None)
        if old is not None:
            os.environ['GML_NO_HEAD_BCE'] = old


class _Epoch(object):
    """one epoch of exp_classify.py:318-369; way: 'plain' | 'static' | 'captured'.  stats [3, 3] on the device: rows train, val,
    test; columns loss, correct, graphs."""

    def __init__(self, dd, which, way, fused, dev, exact=False, seed=0):
        from gnn_matlang_amd import functional as Fn, models
        from gnn_matlang_amd.optim import OneLaunchAdam
        self.dd, self.way, self.fused, self.dev, self.models = dd, way, fused, dev, models
        self.m = _model(which, dev, seed)
        self.opt = OneLaunchAdam(self.m.parameters(), lr=1e-3)
        self.adj = which == 'gnnml1'
        self.bounds = dd.bounds(BS)
        self.scope = lambda: Fn.exact_products(exact)
        self.stats = torch.zeros(3, 3, device=dev)
        self.ev = torch.zeros(3, device=dev)                   # the captured eval forward's sums (copied out per split)
        self.ids_t, self.ids_e = (torch.zeros(BS, dtype=torch.int64, device=dev) for _ in range(2))
        self.gen = torch.Generator().manual_seed(seed)
        self.replay_t = self.replay_e = None
        if way == 'captured':
            self._capture()

    def _batch(self, ids):
        if self.way == 'plain':
            return self.dd.batch(ids)
        return self.dd.batch_assembled(ids, self.bounds, adjacency=self.adj, groups64=True)

    def _train(self, ids, stats):
        with _head(self.fused), self.scope():
            b = self._batch(ids)
            self.opt.zero_grad(set_to_none=True)
            self.models.exp_classify_step_loss(self.m, b, stats=stats).backward()
            self.opt.step()

    def _eval(self, ids, stats):
        with _head(self.fused), self.scope(), torch.no_grad():
            self.models.exp_classify_step_loss(self.m, self._batch(ids), stats=stats)

    def _capture(self):
        """warm-up on a side stream, then one graph per step kind; parameters and optimiser state go back to their initial values"""
        snap = {k: v.clone() for k, v in self.m.state_dict().items()}
        self.ids_t.copy_(torch.arange(400, 400 + BS, device=self.dev))
        self.ids_e.copy_(torch.arange(BS, device=self.dev))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                self._train(self.ids_t, self.stats[0])
                self._eval(self.ids_e, self.ev)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gt, ge = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(gt):
            self._train(self.ids_t, self.stats[0])
        with torch.cuda.graph(ge):
            self._eval(self.ids_e, self.ev)
        with torch.no_grad():
            for k, v in self.m.state_dict().items():
                v.copy_(snap[k])
            for st in self.opt.state.values():
                st['exp_avg'].zero_()
                st['exp_avg_sq'].zero_()
                st['step'].zero_()
        torch.cuda.synchronize()
        self.replay_t, self.replay_e = gt.replay, ge.replay

    def run(self):
        """one epoch; self.stats holds its sums afterwards (nothing is read here)"""
        self.stats.zero_()
        lo, hi = SPLITS['train']
        perm = (torch.randperm(hi - lo, generator=self.gen) + lo).to(self.dev)
        for i in range(0, hi - lo, BS):
            if self.replay_t is not None:
                self.ids_t.copy_(perm[i:i + BS])
                self.replay_t()
            else:
                self._train(perm[i:i + BS].contiguous(), self.stats[0])
        for row, split in ((1, 'val'), (2, 'test')):
            lo, hi = SPLITS[split]
            self.ev.zero_()
            for i in range(lo, hi, BS):
                ids = torch.arange(i, i + BS, device=self.dev)
                if self.replay_e is not None:
                    self.ids_e.copy_(ids)
                    self.replay_e()
                else:
                    self._eval(ids, self.ev)
            self.stats[row].copy_(self.ev)


def _epoch_rows(dd, dev, iters):
    rows = []
    for which in ('gnnml3', 'gnnml1'):
        for way in ('plain', 'static', 'captured'):
            pair = [_Epoch(dd, which, way, fused, dev) for fused in (True, False)]
            for _ in range(2):
                for e in pair:
                    e.run()
            torch.cuda.synchronize()
            t = [[], []]
            for _ in range(iters):                             # alternating: both heads see the same clocks
                for k, e in enumerate(pair):
                    t[k].append(_timed(e.run))
            row = dict(row='epoch', model=which, way=way, steps='16 train + 4 val + 4 test', batch=BS,
                       ms_fused_head=statistics.median(t[0]), ms_torch_head=statistics.median(t[1]), iters=iters)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def _curve_rows(dd, dev, epochs):
    from gnn_matlang_amd import models
    rows = []
    for which in ('gnnml3', 'gnnml1'):
        for exact in (False, True):
            e = _Epoch(dd, which, 'captured', True, dev, exact=exact)
            hist = torch.zeros(epochs, 3, 3, device=dev)
            for k in range(epochs):
                e.run()
                hist[k].copy_(e.stats)                         # device copy: nothing is read per epoch
            torch.cuda.synchronize()
            h = hist.cpu()
            curve = {s: dict(loss=(h[:, r, 0] / h[:, r, 2]).tolist(), acc=models.accuracy_from_stats(h[:, r].t()).tolist())
                     for r, s in enumerate(('train', 'val', 'test'))}
            best = int(torch.argmin(h[:, 1, 0]))               # exp_classify.py:376-378: the test accuracy at the best val loss
            row = dict(row='curve', model=which, arithmetic='exact_products' if exact else 'default', epochs=epochs,
                       final=dict((s, dict(loss=c['loss'][-1], acc=c['acc'][-1])) for s, c in curve.items()),
                       best_val_epoch=best + 1, test_acc_at_best_val=curve['test']['acc'][best], curve=curve)
            rows.append(row)
            print(json.dumps(dict((k, v) for k, v in row.items() if k != 'curve')), flush=True)
    return rows


def _large_rows(dd, dev, iters):
    """one train step on the data set tiled to >= 600,000 nodes, all graphs in one plain batch"""
    from gnn_matlang_amd import models
    from gnn_matlang_amd.optim import OneLaunchAdam
    reps = -(-600000 // int(dd.x.size(0)))
    big = dd.tiled(reps)
    data = big.batch(torch.arange(len(big), device=dev))
    rows = []
    for which in ('gnnml3', 'gnnml1'):
        t = [[], []]
        steps = []
        for fused in (True, False):
            m = _model(which, dev)
            opt = OneLaunchAdam(m.parameters(), lr=1e-3)

            def step(m=m, opt=opt, fused=fused):
                with _head(fused):
                    opt.zero_grad(set_to_none=True)
                    models.exp_classify_step_loss(m, data).backward()
                    opt.step()
            steps.append(step)
        for _ in range(3):
            for s in steps:
                s()
        torch.cuda.synchronize()
        for _ in range(iters):
            for k, s in enumerate(steps):
                t[k].append(_timed(s))
        row = dict(row='large', model=which, graphs=len(big), nodes=int(data.x.size(0)), support_edges=int(data.edge_index2.size(1)),
                   ms_step_fused_head=statistics.median(t[0]), ms_step_torch_head=statistics.median(t[1]), iters=iters)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=200)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_classify.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    dd = _dataset(dev)
    out = dict(device=torch.cuda.get_device_name(0),
               data=dict(graphs=len(dd), nodes=int(dd.x.size(0)), support_edges=int(dd.edge_index2.size(1)), S=int(dd.edge_attr2.size(1)), batch=BS),
               epoch=_epoch_rows(dd, dev, a.iters), large=_large_rows(dd, dev, max(a.iters // 2, 3)), curves=_curve_rows(dd, dev, a.epochs))
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
