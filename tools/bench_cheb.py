"""ChebNet (cheb.ChebConv, functional.ChebConvFunction, csrc/gml_cheb.hip) on the shapes of the experiment scripts:

    layer     ONE layer forward + backward (dW, db and dx; the norm launch INSIDE the window, though a model pays it once for all its
              layers) on the fused road against the torch-op composition (functional.cheb_conv_torch -- what GML_NO_CHEB_FUSED=1
              selects), both roads in ONE process, alternating round by round, every shape warmed, timed with device events around
              synchronised windows; median and 10th / 90th percentiles per road.  Shapes: a ZINC-like batch of 64 at K = 2 (25 -> 64 and 64 -> 64), mutag batch 16
              at K = 3 (7 -> 32, 32 -> 32), sr25 at K = 4 (1 -> 32, 64 -> 64), the 900-node grid at K = 7 (1 -> 64, 64 -> 64), a
              ZINC-like batch tiled to about 500 k rows at K = 2 and K = 5 (64 -> 64).
    wide      the composition ALONE at the 200-wide shapes of ptc_cheb / enzymes_contfeat_cheb (K = 3 on a batch of 64 graphs):
              outside the fused range, the baseline of a later wide kernel.
    step      a whole eager train step (forward, zinc_loss, backward, Adam) of models.zinc_cheb on the ZINC-like batch, both roads.
    seed      a whole expressivity.count_similar seed on sr25 (host clock around the call, which ends in a host read), both roads.
    roof      gml_cheb_fwd alone at the 500 k-row shapes (K = 2: one step launch; K = 5: four): ms, ms per launch, the compulsory
              bytes (per step: the previous Tx once per edge and once per row, Tx_{k-2} and y read from the second step on, Tx_k and y
              written, norm once per edge and row; rowptr and col read once per step) and the flops (2 N K Fin Fout) computed from the
              shapes, against the 8 TB/s HBM roof and the 157.3 TFLOP/s fp32 roof: which roof bounds it and what share is reached.

One JSON line per row; --out (default profiles/cheb.json) writes all of it as one JSON object.

    python tools/bench_cheb.py [--iters 20] [--rounds 4] [--out profiles/cheb.json]
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
ENV = 'GML_NO_CHEB_FUSED'
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


def _lmax(x, ei):
    """the largest eigenvalue of I - D^-1/2 A D^-1/2 (what SpectralDesign stores as lmax), float64 on the host"""
    n = x.shape[0]
    A = np.zeros((n, n))
    ei = np.asarray(ei)
    keep = ei[0] != ei[1]
    np.add.at(A, (ei[1][keep], ei[0][keep]), 1.0)
    A = np.maximum(A, A.T)
    d = A.sum(0)
    dis = np.where(d > 0, 1.0 / np.sqrt(np.maximum(d, 1)), 0.0)
    return np.float32(np.linalg.eigvalsh(np.eye(n) - dis[:, None] * A * dis[None, :]).max())


def _dicts(graphs):
    return [dict(x=x, edge_index=ei, y=y, lmax=_lmax(x, ei)) for x, ei, y in graphs]


def _tiled(batch, reps):
    """(edge_index, N, batch ids, lmax) of the batch repeated reps times"""
    N, B = int(batch.x.size(0)), batch.num_graphs
    dev = batch.x.device
    k = torch.arange(reps, device=dev).view(-1, 1, 1) * N
    ei = (batch.edge_index.unsqueeze(0) + k).permute(1, 0, 2).reshape(2, -1).contiguous()
    bt = (batch.batch.unsqueeze(0) + torch.arange(reps, device=dev).view(-1, 1) * B).reshape(-1)
    return ei, N * reps, bt, batch.lmax.repeat(reps)


def _sets(dev):
    from gnn_matlang_amd import collate, readers, synthetic
    gf = dict(graph_fields=('lmax',))
    zinc = collate(_dicts(synthetic.make_graphs('zinc', 64, seed=0)), **gf).to(dev)
    mutag = collate(_dicts(readers.load_mutag(os.path.join(RAW, 'mutag.mat'))[:16]), **gf).to(dev)
    sr25 = collate(_dicts(readers.load_sr(os.path.join(RAW, 'sr251256.g6'))), **gf).to(dev)
    g = readers.load_twodgrid(os.path.join(RAW, 'TwoDGrid30.mat'))[:1]
    g[0]['lmax'] = _lmax(g[0]['x'], g[0]['edge_index'])
    grid = collate(g, node_fields=('y', 'mask'), **gf).to(dev)
    one = lambda b: (b.edge_index, int(b.x.size(0)), b.batch, b.lmax)
    graphs = dict(zinc64=one(zinc), mutag16=one(mutag), sr25=one(sr25), grid900=one(grid),
                  zinc500k=_tiled(zinc, max(1, round(500000 / int(zinc.x.size(0))))))
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


def _layer(name, graph, Fin, Fout, K, act, rounds, iters, dev, roads=ROADS):
    from gnn_matlang_amd import ChebConv, functional as Fn
    from gnn_matlang_amd.graph import GraphCSR
    ei, N, bt, lam = graph
    torch.manual_seed(0)
    m = ChebConv(Fin, Fout, K).to(dev)
    x = torch.randn(N, Fin, device=dev, requires_grad=True)
    gy = torch.randn(N, Fout, device=dev)
    csr = GraphCSR.from_edge_index(ei, N)
    _road('fused')
    fused = Fn.cheb_conv_supported(x, Fout, K)
    if ('fused' in roads) != fused:
        sys.exit('cheb_conv_supported(%d -> %d, K %d) = %s: not what this row measures' % (Fin, Fout, K, fused))

    def run():
        m.zero_grad(set_to_none=True)
        x.grad = None
        # (the composition takes the edge list it would get from a script; the fused road its CSR, built once per batch as everywhere)
        if os.environ.get(ENV) or not fused:
            y = m(x, ei, batch=bt, lambda_max=lam, act=act, _road='torch')
        else:
            y = m(x, csr, batch=bt, lambda_max=lam, act=act)
        y.backward(gy)

    ms = _alternate(run, rounds, iters, roads=roads)
    kw = dict(set=name, nodes=N, edges=int(ei.size(1)), fin=Fin, fout=Fout, K=K, act=act)
    if 'fused' in roads:
        return _row(ms, row='layer', **kw)
    c = ms['composition']
    return dict(kw, row='wide', composition_ms=round(statistics.median(c), 4), composition_p10_p90=_quant(c), samples=len(c))


def _step(batch, rounds, iters, dev):
    from gnn_matlang_amd import models
    torch.manual_seed(0)
    m = models.zinc_cheb(int(batch.x.size(1))).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)

    def run():
        opt.zero_grad(set_to_none=True)
        models.zinc_loss(m(batch, _road='torch' if os.environ.get(ENV) else None), batch.y).backward()
        opt.step()
    return _row(_alternate(run, rounds, iters), row='step', set='zinc64', graphs=batch.num_graphs, model='zinc_cheb')


def _seed(batch, rounds, iters, dev):
    from gnn_matlang_amd import expressivity, models
    out = {}

    def run():
        out['count'] = expressivity.count_similar(lambda: models.sr25_cheb(int(batch.x.size(1))), batch, seeds=[0])[-1]
    row = _row(_alternate(run, rounds, iters, sync_host=True), row='seed', set='sr25', graphs=batch.num_graphs, model='sr25_cheb')
    row['similar_after_seed0'] = out['count']
    return row


def _roof(graph, Fin, Fout, K, iters, dev):
    """gml_cheb_fwd alone (its K - 1 step launches) at the large shape against both roofs; bytes and flops from the shapes"""
    from gnn_matlang_amd import _lib, functional as Fn
    from gnn_matlang_amd.graph import GraphCSR, _ptr, _stream
    ei, N, bt, lam = graph
    csr = GraphCSR.from_edge_index(ei, N)
    norm = Fn.cheb_norm(csr, bt, lam)
    x = torch.randn(N, Fin, device=dev)
    w, b = torch.randn(K, Fin, Fout, device=dev) * 0.1, torch.randn(Fout, device=dev)
    T, y = torch.empty(N, (K - 1) * Fin, device=dev), torch.empty(N, Fout, device=dev)
    st = _stream(dev)

    def run():
        _lib.call('gml_cheb_fwd', _ptr(csr.rowptr), _ptr(csr.col), _ptr(norm), _ptr(x), Fin, N, csr.E, Fin, _ptr(w), _ptr(b), Fout, K, 1,
                  _ptr(T), (K - 1) * Fin, _ptr(y), Fout, st)
    run()
    tms = _events(run, iters)
    E, steps = csr.E, K - 1
    per_step = (E + N) * Fin + N * Fin + N * Fout + 2 * (E + N) + E + N + 1       # gather, Tx_k out, y out, norm, col and rowptr
    q = 4 * (steps * per_step + N * Fin + (steps - 1) * (N * Fin + N * Fout))     # x for x W_0; Tx_{k-2} and y in from the second step on
    fl = 2 * N * K * Fin * Fout
    med = statistics.median(tms) * 1e-3
    t_hbm, t_fp32 = q / HBM_ROOF, fl / FP32_ROOF
    bound = 'hbm' if t_hbm >= t_fp32 else 'fp32'
    return dict(row='roof', set='zinc500k', kernel='gml_cheb_fwd', nodes=N, edges=E, fin=Fin, fout=Fout, K=K, launches=steps,
                ms=round(med * 1e3, 4), ms_per_launch=round(med * 1e3 / steps, 4), p10_p90=_quant(tms), compulsory_bytes=q, flops=fl,
                tb_per_s=round(q / med / 1e12, 3), tflop_per_s=round(fl / med / 1e12, 2), hbm_roof_ms=round(t_hbm * 1e3, 4),
                fp32_roof_ms=round(t_fp32 * 1e3, 4), bound_by=bound, fraction_of_bounding_roof=round(max(t_hbm, t_fp32) / med, 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cheb.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_cheb.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    graphs, batches = _sets(dev)
    _layer('zinc64', graphs['zinc64'], 25, 64, 2, 'relu', 1, a.iters, dev)           # discarded: the first shape a process measures reads high
    rows = []
    shapes = (('zinc64', 25, 64, 2, 'relu'), ('zinc64', 64, 64, 2, 'relu'), ('mutag16', 7, 32, 3, 'relu'), ('mutag16', 32, 32, 3, 'relu'),
              ('sr25', 1, 32, 4, 'tanh'), ('sr25', 64, 64, 4, 'tanh'), ('grid900', 1, 64, 7, 'relu'), ('grid900', 64, 64, 7, 'relu'),
              ('zinc500k', 64, 64, 2, 'relu'), ('zinc500k', 64, 64, 5, 'relu'))
    for name, Fin, Fout, K, act in shapes:
        big = graphs[name][1] > 100000
        rows.append(_layer(name, graphs[name], Fin, Fout, K, act, a.rounds, max(4, a.iters // 4) if big else a.iters, dev))
        print(json.dumps(rows[-1]), flush=True)
    for name, Fin in (('zinc64', 20), ('zinc64', 22), ('zinc64', 200)):                # the 200-wide ChebNets: the composition alone
        rows.append(_layer(name, graphs[name], Fin, 200, 3, 'relu', a.rounds, a.iters, dev, roads=('composition',)))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(_step(batches['zinc'], a.rounds, a.iters, dev))
    print(json.dumps(rows[-1]), flush=True)
    rows.append(_seed(batches['sr25'], a.rounds, max(3, a.iters // 5), dev))
    print(json.dumps(rows[-1]), flush=True)
    for K in (2, 5):
        rows.append(_roof(graphs['zinc500k'], 64, 64, K, a.iters, dev))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(tool='tools/bench_cheb.py', device=torch.cuda.get_device_name(0),
               what='ms; median of rounds x iters samples per road, roads alternating in one process, every shape warmed; layer, wide and '
                    'step: device-event intervals; seed: host clock around count_similar(seeds=[0]), which ends in a host read; roof: '
                    'gml_cheb_fwd alone against 8 TB/s and 157.3 TFLOP/s',
               launches_per_layer=dict(norm_per_batch=1, fused_forward='K - 1 (1 at K = 1)', fused_backward='K + 1', fused_backward_without_dx=2),
               rounds=a.rounds, iters=a.iters, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
