"""The TF GNNML3 of enzymes_contfeats_gnnml3_tf.py (models.enzymes_contfeat_gnnml3) on the real ENZYMES graphs
(tests/golden/raw/enzymes.mat: 600 graphs of 2 .. 126 nodes, recfield = 5, 97 % full masks, S = 4) and fold 1 of the script's split,
three batches of 180 training graphs per epoch.  Two roads, alternating in one process, device events:

    HIP      dense_block.spectconv_ragged on csrc/gml_dense_rag.hip (bank of bf16 images, compact rows, keep bits in the kernel)
    library  the same layer under functional.exact_products(): torch.bmm in fp32 on blocks padded to 128 + the elementwise mask
             from the SAME keep bits

    layer     one conv layer forward + backward at 22 -> 200 (no dX: the first layer) and 200 -> 200, with and without support dropout
    step      one whole train step (forward, dssgcn_loss, backward, Adam lr 1e-3) in training mode, dropout 0.1
    training  train cross entropy and fold-1 test accuracy after --epochs epochs on each road: recorded, not asserted

One JSON line per row; --out (default profiles/enzymes_contfeat_tf.json) writes all of it as one JSON object.

    python tools/bench_enzymes_tf.py [--epochs 400] [--iters 30] [--out profiles/enzymes_contfeat_tf.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RAW = os.path.join(ROOT, 'tests', 'golden', 'raw')


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(ts):
    return dict(median=float(np.median(ts)), p10=float(np.percentile(ts, 10)), p90=float(np.percentile(ts, 90)))


def _ab(run, iters):
    """run(lib) timed on both roads, alternating: both see the same clocks"""
    from gnn_matlang_amd import functional as Fn

    def road(lib):
        with Fn.exact_products(lib):
            run()
    for _ in range(3):
        road(False)
        road(True)
    torch.cuda.synchronize()
    th, tl = [], []
    for _ in range(iters):
        th.append(_timed(lambda: road(False)))
        tl.append(_timed(lambda: road(True)))
    h, l = _stats(th), _stats(tl)
    return dict(ms_hip=h, ms_library=l, library_over_hip=l['median'] / h['median'])


class Data(object):
    def __init__(self, dev):
        from gnn_matlang_amd import SpectralDesign, collate, dense_block, readers
        raw = readers.load_tu(os.path.join(RAW, 'enzymes.mat'), 'enzymes', contfeat=True)
        self.train = np.loadtxt(os.path.join(RAW, 'enzymes_fold1_train_idx.txt')).astype(np.int64)
        self.test = np.loadtxt(os.path.join(RAW, 'enzymes_fold1_test_idx.txt')).astype(np.int64)
        recs = SpectralDesign(recfield=5, dv=1, nfreq=3, adddegree=True).design_many(raw)
        self.recs, _ = readers.standardize_tu(recs, self.train, ddof=0)
        full = collate(self.recs).to(dev)
        self.bank = dense_block.RaggedSupports(full.edge_index2, full.edge_attr2, full.batch, full.ptr)
        self.dev = dev
        self.nodes, self.entries = int(full.x.size(0)), int(full.edge_index2.size(1))

    def batch(self, ids):
        """the graphs `ids` as one batch: compact node rows + bank slots (the supports stay in the bank)"""
        from gnn_matlang_amd import dense_block
        from gnn_matlang_amd.graph import Batch
        sizes = [self.recs[i]['x'].shape[0] for i in ids]
        b = Batch(x=torch.from_numpy(np.concatenate([self.recs[i]['x'] for i in ids])),
                  batch=torch.from_numpy(np.repeat(np.arange(len(ids)), sizes)),
                  ptr=torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32),
                  y=torch.tensor([int(self.recs[i]['y']) for i in ids])).to(self.dev)
        return dense_block.attach_bank(b, self.bank, torch.tensor(np.asarray(ids), dtype=torch.int32, device=self.dev))

    def epoch(self, rng, nbatch=3):
        """the script's lines 176-186: shuffle the training ids, cut at round(linspace(0, len, nbatch + 1))"""
        ids = rng.permutation(self.train)
        cut = np.round(np.linspace(0, len(ids), nbatch + 1)).astype(int)
        return [self.batch(ids[cut[i]:cut[i + 1]]) for i in range(nbatch)]


def _layers(data, batches, iters):
    from gnn_matlang_amd import dense_block
    from gnn_matlang_amd import functional as Fn
    rows = []
    b = batches[0]
    N = int(b.x.size(0))
    state = Fn.dropout_state(1, data.dev)
    for Fin, Fout in ((22, 200), (200, 200)):
        for p in (0.0, 0.1):
            torch.manual_seed(1)
            x = torch.randn(N, Fin, device=data.dev, requires_grad=Fin != 22)
            w = (torch.rand(4, Fin, Fout, device=data.dev) - 0.5).requires_grad_()
            g = torch.randn(N, Fout, device=data.dev)

            def run():
                x.grad = w.grad = None
                dense_block.spectconv_ragged(x, b.bank, b.gid, b.ptr, w, None, relu=True, p=p, state=state, site=1, training=True).backward(g)
            row = dict(row='layer', Fin=Fin, Fout=Fout, kernel_dropout=p, graphs=b.num_graphs, nodes=N, **_ab(run, iters))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def _model(dev, seed=0):
    from gnn_matlang_amd import models
    torch.manual_seed(seed)
    m = models.enzymes_contfeat_gnnml3().to(dev)
    return m, torch.optim.Adam(m.parameters(), lr=1e-3)


def _train_step(m, opt, b):
    from gnn_matlang_amd import models
    opt.zero_grad(set_to_none=True)
    logits = m(b)
    loss = models.dssgcn_loss(m, logits, b.y)
    loss.backward()
    opt.step()
    return logits


def _step(data, batches, iters):
    m, opt = _model(data.dev)
    m.train()
    k = [0]

    def run():
        _train_step(m, opt, batches[k[0] % len(batches)])
        k[0] += 1
    row = dict(row='step', graphs=[b.num_graphs for b in batches], **_ab(run, 3 * iters))
    print(json.dumps(row), flush=True)
    return row


def _training(data, epochs):
    from gnn_matlang_amd import functional as Fn
    rows = []
    test = data.batch(data.test)
    for lib in (False, True):
        m, opt = _model(data.dev)
        rng = np.random.default_rng(0)
        ent = torch.zeros(3, device=data.dev)
        with Fn.exact_products(lib):
            for _ in range(epochs):
                m.train()
                for i, b in enumerate(data.epoch(rng)):
                    logits = _train_step(m, opt, b)
                    ent[i] = torch.nn.functional.cross_entropy(logits.detach(), b.y)
            m.eval()
            with torch.no_grad():
                acc = float((m(test).argmax(1) == test.y).float().mean())
        row = dict(row='training', road='library' if lib else 'HIP', epochs=epochs, train_xent=float(ent.mean()), test_acc_fold1=acc)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=400)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'enzymes_contfeat_tf.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    data = Data(dev)
    batches = data.epoch(np.random.default_rng(0))
    sizes = np.asarray(data.bank.sizes)
    out = dict(device=torch.cuda.get_device_name(0),
               data=dict(graphs=int(sizes.size), nodes=data.nodes, mask_entries=data.entries, sum_n2=int((sizes ** 2).sum()),
                         padded_read_fraction=float((sizes ** 2).sum()) / (sizes.size * float(sizes.max()) ** 2)),
               layers=_layers(data, batches, a.iters), step=_step(data, batches, a.iters), training=_training(data, a.epochs))
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
