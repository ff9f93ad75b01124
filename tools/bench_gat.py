"""GAT (gat.GATConv, functional.GATConvFunction, csrc/gml_gat.hip) on the shapes of the experiment scripts:

    layer     ONE layer forward + backward (all parameter gradients and dx) on the fused road against the torch-op composition
              (functional.gat_conv_torch -- what GML_NO_GAT_FUSED=1 selects), both roads in ONE process, alternating round by round,
              timed with device events; median and 10th / 90th percentiles per road, and the launches of one forward + backward per
              road (torch profiler; null when unavailable).  Shapes: a ZINC-like batch of 64 (25 -> 8 x 8 and 96 -> 8 x 12), mutag
              batch 16, sr25 (15 graphs of 25 nodes, degree 12), the 900-node grid, a ZINC-like batch tiled to about 500 k rows.
    step      a whole eager train step (forward, zinc_loss, backward, Adam) of models.zinc_gat on the ZINC-like batch, both roads.
    seed      a whole expressivity.count_similar seed on sr25 (host clock around the call, which ends in a host read), both roads.
    roof      gml_gat_fwd alone at the 500 k-row shape: ms, the compulsory bytes (xl read once per edge, the self edge included, and
              y written once) and the fraction of the 8 TB/s HBM roof they reach.

One JSON line per row; --out (default profiles/gat.json) writes all of it as one JSON object.

    python tools/bench_gat.py [--iters 20] [--rounds 4] [--out profiles/gat.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RAW = os.path.join(ROOT, 'tests', 'golden', 'raw')
ENV = 'GML_NO_GAT_FUSED'
ROADS = ('fused', 'composition')
HBM_ROOF = 8.0e12


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


def _launches(run):
    try:
        from torch.profiler import profile, ProfilerActivity
        run()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            run()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e, 'device_type', None) is not None and 'cuda' in str(e.device_type).lower())
        return n or None
    except Exception:
        return None


def _alternate(run, rounds, iters, sync_host=False):
    """ms per call of run(), per road: round 0 warms both roads up; roads alternate round by round"""
    ms = {r: [] for r in ROADS}
    for rnd in range(rounds + 1):
        for road in ROADS:
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
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
                ev[0].record()
                for i in range(iters):
                    run()
                    ev[i + 1].record()
                torch.cuda.synchronize()
                t = [ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]
            if rnd:
                ms[road] += t
    _road('fused')
    return ms


def _row(ms, **kw):
    f, c = statistics.median(ms['fused']), statistics.median(ms['composition'])
    fq, cq = _quant(ms['fused']), _quant(ms['composition'])
    return dict(kw, fused_ms=round(f, 4), composition_ms=round(c, 4), speedup=round(c / f, 2), fused_p10_p90=fq, composition_p10_p90=cq,
                fused_p90_below_composition_p10=bool(fq[1] < cq[0]), samples=len(ms['fused']))


def _layer(name, ei, N, Fin, C, act, rounds, iters, dev):
    from gnn_matlang_amd import GATConv, functional as Fn
    from gnn_matlang_amd.graph import GraphCSR
    torch.manual_seed(0)
    m = GATConv(Fin, C, heads=8).to(dev)
    x = torch.randn(N, Fin, device=dev, requires_grad=True)
    gy = torch.randn(N, 8 * C, device=dev)
    csr = GraphCSR.from_edge_index(ei, N)
    _road('fused')
    if not Fn.gat_conv_supported(x, 8, C):
        sys.exit('the library does not serve the GAT layer at 8 x %d' % C)

    def run():
        m.zero_grad(set_to_none=True)
        x.grad = None
        # (the composition takes the edge list it would get from a script; the fused road its CSR, built once per batch as everywhere)
        y = m(x, ei, act=act, _road='torch') if os.environ.get(ENV) else m(x, csr, act=act)
        y.backward(gy)

    launches = {}
    for road in ROADS:
        _road(road)
        launches[road] = _launches(run)
    ms = _alternate(run, rounds, iters)
    return _row(ms, row='layer', set=name, nodes=N, edges=int(ei.size(1)), fin=Fin, heads=8, c=C, act=act, launches_fused=launches['fused'],
                launches_composition=launches['composition'])


def _step(batch, rounds, iters, dev):
    from gnn_matlang_amd import models
    torch.manual_seed(0)
    m = models.zinc_gat(int(batch.x.size(1))).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)

    def run():
        opt.zero_grad(set_to_none=True)
        models.zinc_loss(m(batch, _road='torch' if os.environ.get(ENV) else None), batch.y).backward()
        opt.step()
    return _row(_alternate(run, rounds, iters), row='step', set='zinc64', graphs=batch.num_graphs, model='zinc_gat')


def _seed(batch, rounds, iters, dev):
    from gnn_matlang_amd import expressivity, models
    out = {}
    factory = lambda: models.sr25_gat(int(batch.x.size(1)))

    def run():
        out['count'] = expressivity.count_similar(factory, batch, seeds=[0])[-1]
    row = _row(_alternate(run, rounds, iters, sync_host=True), row='seed', set='sr25', graphs=batch.num_graphs, model='sr25_gat')
    row['similar_after_seed0'] = out['count']
    return row


def _roof(ei, N, C, iters, dev):
    """gml_gat_fwd alone (the aggregation launch) at the large shape"""
    from gnn_matlang_amd import _lib
    from gnn_matlang_amd.graph import GraphCSR, _ptr, _stream
    HC = 8 * C
    csr = GraphCSR.from_edge_index(ei, N)
    xl, b = torch.randn(N, HC, device=dev), torch.randn(HC, device=dev)
    att = torch.randn(2, HC, device=dev) * 0.3
    al, ar, m, z = (torch.empty(N, 8, device=dev) for _ in range(4))
    y = torch.empty(N, HC, device=dev)
    st = _stream(dev)
    _lib.call('gml_gat_logits', _ptr(xl), HC, _ptr(att[0]), _ptr(att[1]), N, 8, C, _ptr(al), _ptr(ar), st)

    def run():
        _lib.call('gml_gat_fwd', _ptr(csr.rowptr), _ptr(csr.col), _ptr(xl), HC, _ptr(al), _ptr(ar), _ptr(b), N, csr.E, 8, C, 3, _ptr(y), HC,
                  _ptr(m), _ptr(z), st)
    run()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        run()
        ev[i + 1].record()
    torch.cuda.synchronize()
    t = [ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]
    nself = int((ei[0] == ei[1]).sum())
    q = 4 * ((csr.E - nself + N) * HC + N * HC)
    med = statistics.median(t)
    return dict(row='roof', set='zinc500k', kernel='gml_gat_fwd', nodes=N, edges=csr.E, c=C, ms=round(med, 4), p10_p90=_quant(t),
                compulsory_bytes=q, tb_per_s=round(q / (med * 1e-3) / 1e12, 3), fraction_of_8tb_roof=round(q / (med * 1e-3) / HBM_ROOF, 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gat.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_gat.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    graphs, batches = _sets(dev)
    _layer('zinc64', *graphs['zinc64'], 25, 8, 'elu', 1, a.iters, dev)          # discarded: the first shape a process measures reads high
    rows = []
    shapes = (('zinc64', 25, 8, 'elu'), ('zinc64', 96, 12, 'elu'), ('mutag16', 8, 8, 'elu'), ('mutag16', 128, 16, 'elu'),
              ('sr25', 2, 16, 'tanh'), ('sr25', 128, 16, 'tanh'), ('grid900', 1, 16, 'elu'), ('grid900', 128, 16, 'elu'),
              ('zinc500k', 25, 8, 'elu'), ('zinc500k', 96, 12, 'elu'))
    for name, Fin, C, act in shapes:
        big = graphs[name][1] > 100000
        rows.append(_layer(name, *graphs[name], Fin, C, act, a.rounds, max(4, a.iters // 4) if big else a.iters, dev))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(_step(batches['zinc'], a.rounds, a.iters, dev))
    print(json.dumps(rows[-1]), flush=True)
    rows.append(_seed(batches['sr25'], a.rounds, max(3, a.iters // 5), dev))
    print(json.dumps(rows[-1]), flush=True)
    rows.append(_roof(*graphs['zinc500k'], 12, a.iters, dev))
    print(json.dumps(rows[-1]), flush=True)
    out = dict(tool='tools/bench_gat.py', device=torch.cuda.get_device_name(0),
               what='ms; median of rounds x iters samples per road, roads alternating in one process; layer and step: device-event '
                    'intervals; seed: host clock around count_similar(seeds=[0]), which ends in a host read; roof: gml_gat_fwd alone',
               launches_per_layer=dict(fused_forward=3, fused_backward=6, of_which_library_gemms=dict(forward=1, backward=2)),
               rounds=a.rounds, iters=a.iters, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
