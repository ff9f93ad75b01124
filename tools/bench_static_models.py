"""mutag at the reference's batch size (bsize = 16, mutag.py:320-351) on the real graphs (tests/golden/raw/mutag.mat), for mutag GNNML3
and mutag GNNML1 (models.mutag_gnnml1), three ways each:
    eager   over DeviceDataset.epoch()          plain batches, per-batch CSR build with host reads
    static  over DeviceDataset.epoch_static()   padded batches from gml_batch_assemble (+ _edges), masked BatchNorm, no host read
    graph   one captured step replayed per batch (assembly + forward + masked loss + backward + running statistics + OneLaunchAdam)
Reports ms/step and the summed loss of every timed epoch (one JSON line per model and way; --out FILE also writes them as a JSON
list).  Every way starts from the same parameters and trains one warm-up epoch before the timed ones; the captured way also trains
through its three warm-up steps and the capture step, so its losses run a few steps ahead of the other two.

    python tools/bench_static_models.py [--epochs 5] [--out profiles/static_models_mutag_bs16.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=5, help='timed epochs per way (after one warm-up epoch)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from gnn_matlang_amd import SpectralDesign, models, readers
    from gnn_matlang_amd.dataset import DeviceDataset
    from gnn_matlang_amd.optim import OneLaunchAdam
    dev = torch.device('cuda:0')
    raw = readers.load_mutag(os.path.join(ROOT, 'tests', 'golden', 'raw', 'mutag.mat'))
    dd = DeviceDataset.from_graphs(SpectralDesign(recfield=1, dv=4, nfreq=3, adddegree=True).design_many(raw), dev)   # mutag.py:14
    dd.y = dd.y.float()
    dd.prepare()
    G = len(dd)
    bd = dd.bounds(BS)
    ctors = {'mutag_gnnml3': lambda: models.mutag_gnnml3(), 'mutag_gnnml1': lambda: models.mutag_gnnml1()}
    rows = []
    for name, ctor in ctors.items():
        adj = name == 'mutag_gnnml1'
        for way in ('eager', 'static', 'graph'):
            torch.manual_seed(0)
            m = ctor().to(dev).train()
            opt = OneLaunchAdam(m.parameters(), lr=1e-3)
            gen = torch.Generator().manual_seed(1)
            tot = torch.zeros((), device=dev)

            def one(b):
                opt.zero_grad(set_to_none=True)
                l = models.mutag_step_loss(m, b)
                l.backward()
                opt.step()
                tot.add_(l.detach())
            if way == 'eager':
                def epoch():
                    n = 0
                    for b in dd.epoch(BS, generator=gen):
                        one(b)
                        n += 1
                    return n
            elif way == 'static':
                def epoch():
                    n = 0
                    for b in dd.epoch_static(BS, generator=gen, bounds=bd, adjacency=adj, groups64=True):
                        one(b)
                        n += 1
                    return n
            else:
                ids_buf = torch.arange(BS, dtype=torch.int64, device=dev)

                def step():
                    one(dd.batch_assembled(ids_buf, bd, adjacency=adj, groups64=True))
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
                    perm = torch.cat([perm, torch.full(((-G) % BS,), G, dtype=torch.int64, device=dev)])
                    for i in range(0, perm.numel(), BS):
                        ids_buf.copy_(perm[i:i + BS])
                        graph.replay()
                    return perm.numel() // BS
            epoch()                                                        # warm-up epoch
            torch.cuda.synchronize()
            losses, steps, secs = [], 0, 0.0
            for _ in range(args.epochs):
                tot.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps_e = epoch()
                torch.cuda.synchronize()
                secs += time.perf_counter() - t0
                steps += steps_e
                losses.append(float(tot.item()))
            row = dict(model=name, way=way, batch_size=BS, graphs=G, steps_per_epoch=steps // args.epochs, epochs=args.epochs,
                       ms_per_step=secs / steps * 1e3, epoch_loss=losses,
                       bounds=dict(n_pad=bd['n_pad'], e2_pad=bd['e2_pad'], e_pad=bd['e_pad']))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
