"""GIN (gin.GINConv, functional.GINConvFunction, csrc/gml_gin.hip) on the shapes of the experiment scripts:

    layer     ONE layer forward + backward (all parameter gradients, deps and dx) on the fused road against the torch-op composition
              (functional.gin_conv_torch -- what GML_NO_GIN_FUSED=1 selects), both roads in ONE process, alternating round by round,
              every shape warmed, timed with device events around synchronised windows; median and 10th / 90th percentiles per road.
              Shapes: a ZINC-like batch of 64 (25 -> 64 -> 64 and 64 -> 64 -> 64), mutag batch 16, sr25 at depth 1, the 900-node grid
              at 1 -> 64 -> 64, a ZINC-like batch tiled to about 500 k rows at both ZINC shapes.
    wide      the composition ALONE at the 200-wide shapes of ptc_gin / enzymes_contfeat_gin (20 | 22 -> 200 -> 200 and
              200 -> 200 -> 200 on a batch of 64 graphs): outside the fused range, the baseline of a later 200-wide kernel.
    step      a whole eager train step (forward, zinc_loss, backward, Adam) of models.zinc_gin on the ZINC-like batch, both roads.
    seed      a whole expressivity.count_similar seed on sr25 (host clock around the call, which ends in a host read), both roads.
    roof      gml_gin_fwd alone at the 500 k-row shapes: ms, the compulsory bytes (x read once per edge and once per row, h, t and y
              written once, rowptr and col read once) and the flops (2 N (Fin Fh + Fh Fout)) computed from the shapes, against the
              8 TB/s HBM roof and the 157.3 TFLOP/s fp32 roof: which roof bounds the launch and what share of it is reached.

One JSON line per row; --out (default profiles/gin.json) writes all of it as one JSON object.

    python tools/bench_gin.py [--iters 20] [--rounds 4] [--out profiles/gin.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RAW = os.path.join(ROOT, 'tests', 'golden', 'raw')
ENV = 'GML_NO_GIN_FUSED'
ROADS = ('fused', 'composition')
HBM_ROOF = 8.0e12
FP32_ROOF = 157.3e12


def _road(road):
    if road == 'composition':
        os.environ[ENV] = '1'
    else:
        os.environ.pop(ENV, None)


def _quant(v):
    return [round(statistics.quantiles(v, n=10)[i], 4) for i in (0, 8)]


def _dicts(graphs):
    return [dict(x=x, edge_index=ei, y=y) for x, ei, y in graphs]


def _tiled(batch, reps):
    """(edge_index, N) of the batch repeated reps times"""
    N = int(batch.x.size(0))
    k = torch.arange(reps, device=batch.x.device).view(-1, 1, 1) * N
    return (batch.edge_index.unsqueeze(0) + k).permute(1, 0, 2).reshape(2, -1).contiguous(), N * reps


def _sets(dev):
    from gnn_matlang_amd import collate, readers, synthetic
    zinc = collate(_dicts(synthetic.make_graphs('zinc', 64, seed=0))).to(dev)
    mutag = collate(_dicts(readers.load_mutag(os.path.join(RAW, 'mutag.mat'))[:16])).to(dev)
    sr25 = collate(_dicts(readers.load_sr(os.path.join(RAW, 'sr251256.g6')))).to(dev)
    grid = collate(readers.load_twodgrid(os.path.join(RAW, 'TwoDGrid30.mat'))[:1], node_fields=('y', 'mask')).to(dev)
    big = _tiled(zinc, max(1, round(500000 / int(zinc.x.size(0)))))
    graphs = dict(zinc64=(zinc.edge_index, int(zinc.x.size(0))), mutag16=(mutag.edge_index, int(mutag.x.size(0))),
                  sr25=(sr25.edge_index, int(sr25.x.size(0))), grid900=(grid.edge_index, int(grid.x.size(0))), zinc500k=big)
    return graphs, dict(zinc=zinc, sr25=sr25)


def _events(run, iters):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(iters):
        run()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]


def _alternate(run, rounds, iters, sync_host=False, roads=ROADS):
    """ms per call of run(), per road: round 0 warms every road up; roads alternate round by round"""
    ms = {r: [] for r in roads}
    for rnd in range(rounds + 1):
        for road in roads:
            _road(road)
            run()
            torch.cuda.synchronize()
            if sync_host:
                t = []
                for _ in range(iters):
                    t0 = time.perf_counter()
                    run()
                    torch.cuda.synchronize()
                    t.append((time.perf_counter() - t0) * 1e3)
            else:
                t = _events(run, iters)
            if rnd:
                ms[road] += t
    _road('fused')
    return ms


def _row(ms, **kw):
    f, c = statistics.median(ms['fused']), statistics.median(ms['composition'])
    fq, cq = _quant(ms['fused']), _quant(ms['composition'])
    return dict(kw, fused_ms=round(f, 4), composition_ms=round(c, 4), speedup=round(c / f, 2), fused_p10_p90=fq, composition_p10_p90=cq,
                fused_p90_below_composition_p10=bool(fq[1] < cq[0]), samples=len(ms['fused']))


def _module(Fin, width, depth, dev):
    from gnn_matlang_amd import GINConv
    from torch.nn import Linear, ReLU, Sequential
    nn = Sequential(Linear(Fin, width), ReLU(), Linear(width, width)) if depth == 2 else Sequential(Linear(Fin, width))
    return GINConv(nn, eps=0.1, train_eps=True).to(dev)


def _layer(name, ei, N, Fin, width, depth, act, rounds, iters, dev, roads=ROADS):
    from gnn_matlang_amd import functional as Fn
    from gnn_matlang_amd.graph import GraphCSR
    torch.manual_seed(0)
    m = _module(Fin, width, depth, dev)
    x = torch.randn(N, Fin, device=dev, requires_grad=True)
    gy = torch.randn(N, width, device=dev)
    csr = GraphCSR.from_edge_index(ei, N)
    _road('fused')
    fused = Fn.gin_conv_supported(x, width, width if depth == 2 else None)
    if ('fused' in roads) != fused:
        sys.exit('gin_conv_supported(%d -> %d, depth %d) = %s: not what this row measures' % (Fin, width, depth, fused))

    def run():
        m.zero_grad(set_to_none=True)
        x.grad = None
        # (the composition takes the edge list it would get from a script; the fused road its CSR, built once per batch as everywhere)
        y = m(x, ei, act=act, _road='torch') if (os.environ.get(ENV) or not fused) else m(x, csr, act=act)
        y.backward(gy)

    ms = _alternate(run, rounds, iters, roads=roads)
    kw = dict(set=name, nodes=N, edges=int(ei.size(1)), fin=Fin, width=width, depth=depth, act=act)
    if 'fused' in roads:
        return _row(ms, row='layer', **kw)
    c = ms['composition']
    return dict(kw, row='wide', composition_ms=round(statistics.median(c), 4), composition_p10_p90=_quant(c), samples=len(c))


def _step(batch, rounds, iters, dev):
    from gnn_matlang_amd import models
    torch.manual_seed(0)
    m = models.zinc_gin(int(batch.x.size(1))).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)

    def run():
        opt.zero_grad(set_to_none=True)
        models.zinc_loss(m(batch, _road='torch' if os.environ.get(ENV) else None), batch.y).backward()
        opt.step()
    return _row(_alternate(run, rounds, iters), row='step', set='zinc64', graphs=batch.num_graphs, model='zinc_gin')


def _seed(batch, rounds, iters, dev):
    from gnn_matlang_amd import expressivity, models
    out = {}

    def factory():
        np.random.seed(0)
        return models.sr25_gin(int(batch.x.size(1)))

    def run():
        out['count'] = expressivity.count_similar(factory, batch, seeds=[0])[-1]
    row = _row(_alternate(run, rounds, iters, sync_host=True), row='seed', set='sr25', graphs=batch.num_graphs, model='sr25_gin')
    row['similar_after_seed0'] = out['count']
    return row


def _roof(ei, N, Fin, width, iters, dev):
    """gml_gin_fwd alone (depth 2) at the large shape against both roofs; bytes and flops from the shapes"""
    from gnn_matlang_amd import _lib
    from gnn_matlang_amd.graph import GraphCSR, _ptr, _stream
    csr = GraphCSR.from_edge_index(ei, N)
    x = torch.randn(N, Fin, device=dev)
    w1, b1 = torch.randn(width, Fin, device=dev) * 0.1, torch.randn(width, device=dev)
    w2, b2 = torch.randn(width, width, device=dev) * 0.1, torch.randn(width, device=dev)
    eps = torch.full((1,), 0.1, device=dev)
    h, t, y = torch.empty(N, Fin, device=dev), torch.empty(N, width, device=dev), torch.empty(N, width, device=dev)
    st = _stream(dev)

    def run():
        _lib.call('gml_gin_fwd', _ptr(csr.rowptr), _ptr(csr.col), _ptr(x), Fin, N, csr.E, Fin, _ptr(eps), _ptr(w1), _ptr(b1), width, _ptr(w2),
                  _ptr(b2), width, 2, 1, _ptr(h), Fin, _ptr(t), width, _ptr(y), width, st)
    run()
    tms = _events(run, iters)
    q = 4 * ((csr.E + N) * Fin + N * (Fin + 2 * width) + csr.E + N + 1)
    fl = 2 * N * (Fin * width + width * width)
    med = statistics.median(tms) * 1e-3
    t_hbm, t_fp32 = q / HBM_ROOF, fl / FP32_ROOF
    bound = 'hbm' if t_hbm >= t_fp32 else 'fp32'
    return dict(row='roof', set='zinc500k', kernel='gml_gin_fwd', nodes=N, edges=csr.E, fin=Fin, width=width, depth=2, ms=round(med * 1e3, 4),
                p10_p90=_quant(tms), compulsory_bytes=q, flops=fl, tb_per_s=round(q / med / 1e12, 3), tflop_per_s=round(fl / med / 1e12, 2),
                hbm_roof_ms=round(t_hbm * 1e3, 4), fp32_roof_ms=round(t_fp32 * 1e3, 4), bound_by=bound,
                fraction_of_bounding_roof=round(max(t_hbm, t_fp32) / med, 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gin.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_gin.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    graphs, batches = _sets(dev)
    _layer('zinc64', *graphs['zinc64'], 25, 64, 2, 'relu', 1, a.iters, dev)          # discarded: the first shape a process measures reads high
    rows = []
    shapes = (('zinc64', 25, 64, 2, 'relu'), ('zinc64', 64, 64, 2, 'relu'), ('mutag16', 7, 64, 2, 'relu'), ('mutag16', 64, 64, 2, 'relu'),
              ('sr25', 1, 64, 1, 'tanh'), ('sr25', 64, 64, 1, 'tanh'), ('grid900', 1, 64, 2, 'relu'), ('grid900', 64, 64, 2, 'relu'),
              ('zinc500k', 25, 64, 2, 'relu'), ('zinc500k', 64, 64, 2, 'relu'))
    for name, Fin, w, depth, act in shapes:
        big = graphs[name][1] > 100000
        rows.append(_layer(name, *graphs[name], Fin, w, depth, act, a.rounds, max(4, a.iters // 4) if big else a.iters, dev))
        print(json.dumps(rows[-1]), flush=True)
    for name, Fin in (('zinc64', 20), ('zinc64', 22), ('zinc64', 200)):                # the 200-wide GinNets: the composition alone
        rows.append(_layer(name, *graphs[name], Fin, 200, 2, 'relu', a.rounds, a.iters, dev, roads=('composition',)))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(_step(batches['zinc'], a.rounds, a.iters, dev))
    print(json.dumps(rows[-1]), flush=True)
    rows.append(_seed(batches['sr25'], a.rounds, max(3, a.iters // 5), dev))
    print(json.dumps(rows[-1]), flush=True)
    for Fin in (25, 64):
        rows.append(_roof(*graphs['zinc500k'], Fin, 64, a.iters, dev))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(tool='tools/bench_gin.py', device=torch.cuda.get_device_name(0),
               what='ms; median of rounds x iters samples per road, roads alternating in one process, every shape warmed; layer, wide and '
                    'step: device-event intervals; seed: host clock around count_similar(seeds=[0]), which ends in a host read; roof: '
                    'gml_gin_fwd alone against 8 TB/s and 157.3 TFLOP/s',
               launches_per_layer=dict(fused_forward=1, fused_backward=3, fused_backward_without_dx=2),
               rounds=a.rounds, iters=a.iters, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
