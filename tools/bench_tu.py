"""Device dropout and the TU GNNML3 models (ptc.py, enzymes.py) on the real graphs (tests/golden/raw/{ptc,enzymes}.mat):

    kernels   gml_dropout_fwd / gml_dropout_bwd alone at [3,005,312 x 32] (the width of bench.py's ZINC batch) and [3,005,312 x 80]:
              ms per launch (HIP events around --iters back-to-back launches) and GB/s on the algorithmic bytes 8 N C + N C / 8
    ptc       train-step ms at the reference's batch 32 (ptc.py:398), dropout 0.2 vs 0.0: eager over DeviceDataset.epoch() (plain batches)
              and as one captured step (assembly, forward, masked NLL, backward, OneLaunchAdam) replayed over batch_assembled batches
    enzymes   eager train-step ms at batch 60, dropout 0.1

One JSON line per row; --out (default profiles/tu_models.json) writes them as one JSON list.

    python tools/bench_tu.py [--epochs 3] [--iters 20] [--out profiles/tu_models.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ZINC = 3005312


def _kernels(dev, iters):
    from gnn_matlang_amd import functional as Fn
    rows = []
    st = Fn.dropout_state(1, dev)
    for C in (32, 80):
        x = torch.randn(N_ZINC, C, device=dev)
        g = torch.randn(N_ZINC, C, device=dev)
        nbytes = 8 * N_ZINC * C + N_ZINC * C // 8
        _, mask = Fn.dropout_fwd(x, 0.2, st, 0)
        for kind in ('fwd', 'bwd'):
            run = (lambda: Fn.dropout_fwd(x, 0.2, st, 0)) if kind == 'fwd' else (lambda: Fn.dropout_bwd(g, mask, 0.2))
            for _ in range(3):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / iters
            row = dict(kernel='gml_dropout_' + kind, N=N_ZINC, C=C, p=0.2, ms=ms, algorithmic_bytes=nbytes, GBps=nbytes / ms / 1e6)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del x, g, mask
    torch.cuda.empty_cache()
    return rows


def _dataset(name, dev):
    from gnn_matlang_amd import SpectralDesign, readers
    from gnn_matlang_amd.dataset import DeviceDataset
    sd = dict(ptc=dict(nmax=109, adddegree=True, recfield=1, dv=10, nfreq=10),          # ptc.py:16
              enzymes=dict(nmax=126, adddegree=True, recfield=1, dv=2, nfreq=4))[name]    # enzymes.py:27
    raw = readers.load_tu(os.path.join(ROOT, 'tests', 'golden', 'raw', '%s.mat' % name), name)
    dd = DeviceDataset.from_graphs(SpectralDesign(**sd).design_many(raw), dev)
    dd.y = dd.y.float()
    dd.prepare()
    return dd


def _train(name, dd, dev, bs, way, dropout, epochs):
    from gnn_matlang_amd import models
    from gnn_matlang_amd.optim import OneLaunchAdam
    torch.manual_seed(0)
    m = getattr(models, name + '_gnnml3')(dropout=dropout).to(dev).train()
    opt = OneLaunchAdam(m.parameters(), lr=1e-3)
    gen = torch.Generator().manual_seed(1)
    tot = torch.zeros((), device=dev)
    G = len(dd)

    def one(b):
        opt.zero_grad(set_to_none=True)
        l = models.tu_step_loss(m, b)
        l.backward()
        opt.step()
        tot.add_(l.detach())
    if way == 'eager':
        def epoch():
            n = 0
            for b in dd.epoch(bs, generator=gen):
                one(b)
                n += 1
            return n
    else:
        bd = dd.bounds(bs)
        ids_buf = torch.arange(bs, dtype=torch.int64, device=dev)

        def step():
            one(dd.batch_assembled(ids_buf, bd, groups64=True))      # (the 64-row records the layers read)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()

        def epoch():
            perm = torch.randperm(G, generator=gen).to(dev)
            perm = torch.cat([perm, torch.full(((-G) % bs,), G, dtype=torch.int64, device=dev)])
            for i in range(0, perm.numel(), bs):
                ids_buf.copy_(perm[i:i + bs])
                graph.replay()
            return perm.numel() // bs
    epoch()                                                                # warm-up epoch
    torch.cuda.synchronize()
    losses, steps, secs = [], 0, 0.0
    for _ in range(epochs):
        tot.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps += epoch()
        torch.cuda.synchronize()
        secs += time.perf_counter() - t0
        losses.append(float(tot.item()))
    row = dict(model=name + '_gnnml3', way=way, dropout=dropout, batch_size=bs, graphs=G, epochs=epochs, steps=steps,
               ms_per_step=secs / steps * 1e3, epoch_loss=losses)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=3, help='timed epochs per row (after one warm-up epoch)')
    ap.add_argument('--iters', type=int, default=20, help='timed launches per kernel row')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tu_models.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_tu measures on the MI355X'
    dev = torch.device('cuda:0')
    rows = _kernels(dev, args.iters)
    ptc = _dataset('ptc', dev)
    for way in ('eager', 'graph'):
        for p in (0.2, 0.0, 0.2, 0.0):                                     # alternated: the spread shows in the repeats
            rows.append(_train('ptc', ptc, dev, 32, way, p, args.epochs))
    enz = _dataset('enzymes', dev)
    for p in (0.1, 0.0):
        rows.append(_train('enzymes', enz, dev, 60, 'eager', p, args.epochs))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
