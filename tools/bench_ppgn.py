"""PPGN (models.PPGN, functional.PPGNBlockFunction, csrc/gml_ppgn.hip) on the shapes of the experiment scripts:

    block     ONE block forward + backward (all parameter gradients; dx for the inner blocks, none for the first block whose input is
              data) on the fused road against the torch-op composition (functional.ppgn_block_torch -- what GML_NO_PPGN_FUSED=1
              selects), both roads in ONE process, alternating round by round, timed with device events; median and 10th / 90th
              percentiles per road, and the launches of one forward + backward per road (torch profiler; null when unavailable).
              Shapes: sr25 (15 graphs, n = 25), graph8c (all 11,117 graphs, n = 8), EXP (1,200 graphs, nmax = 64), a ZINC-like batch of
              64 at nmax = 37 (synthetic).
    step      a whole train step (forward, zinc_loss, backward, Adam) of models.zinc_ppgn on the ZINC-like batch, both roads.
    seed      a whole expressivity.count_similar seed (model construction, forward of the whole set, pair bitmap, count; host clock
              around the call, which ends in a host read) for sr25, graph8c and EXP, both roads.

One JSON line per row; --out (default profiles/ppgn.json) writes all of it as one JSON object.

    python tools/bench_ppgn.py [--iters 20] [--rounds 4] [--out profiles/ppgn.json]
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
ENV = 'GML_NO_PPGN_FUSED'
ROADS = ('fused', 'composition')


def _road(road):
    if road == 'composition':
        os.environ[ENV] = '1'
    else:
        os.environ.pop(ENV, None)


def _quant(v):
    return [round(statistics.quantiles(v, n=10)[i], 4) for i in (0, 8)]


def _dicts(graphs):
    return [dict(x=x, edge_index=ei, y=y) for x, ei, y in graphs]


def _sets(dev):
    from gnn_matlang_amd import collate, ppgn, readers, synthetic
    sets = dict(sr25=(_dicts(readers.load_sr(os.path.join(RAW, 'sr251256.g6'))), 25, 1),
                graph8c=(_dicts(readers.load_graph8c(os.path.join(RAW, 'graph8c.g6'))), 8, 1),
                exp=(_dicts(readers.load_exp(os.path.join(RAW, 'exp.npz'))), 64, 1),
                zinc=(_dicts(synthetic.make_graphs('zinc', 64, seed=0)), 37, 21))
    return {k: ppgn.attach(collate(gs).to(dev), nmax, nfeat) for k, (gs, nmax, nfeat) in sets.items()}


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


def _block(name, batch, C, first, bias, rounds, iters, dev):
    from gnn_matlang_amd import functional as Fn
    n = batch.ppgn_n
    B, nmax = int(batch.X2.size(0)), int(batch.X2.size(-1))
    torch.manual_seed(0)
    if first:
        x = batch.X2
    else:                                                      # an inner block's input: the previous block's output
        m0 = torch.nn.Conv2d(batch.X2.size(1), C, 1).to(dev)
        with torch.no_grad():
            x = Fn.ppgn_block_torch(batch.X2, n, m0.weight, m0.bias, m0.weight, m0.bias,
                                    torch.nn.Conv2d(C + batch.X2.size(1), C, 1).to(dev).weight, None)[0]
        x = x.detach().requires_grad_(True)
    Cin = int(x.size(1))
    ms_ = [torch.nn.Conv2d(Cin, C, 1, bias=bias), torch.nn.Conv2d(Cin, C, 1, bias=bias), torch.nn.Conv2d(C + Cin, C, 1, bias=bias)]
    m1, m2, m3 = (m.to(dev) for m in ms_)
    gy, gr = torch.randn(B, C, nmax, nmax, device=dev), torch.randn(B, 2 * C, device=dev)
    params = [p for m in (m1, m2, m3) for p in m.parameters()]
    _road('fused')
    if not Fn.ppgn_block_supported(x, nmax, Cin, C):
        sys.exit('the library does not serve the PPGN block at nmax = %d, %d -> %d' % (nmax, Cin, C))

    def run():
        for q in params:
            q.grad = None
        x.grad = None
        args = (x, n, m1.weight, m1.bias, m2.weight, m2.bias, m3.weight, m3.bias, 'sum')
        y, r = Fn.ppgn_block_torch(*args) if os.environ.get(ENV) else Fn.PPGNBlockFunction.apply(*args)
        torch.autograd.backward((y, r), (gy, gr))

    launches = {}
    for road in ROADS:
        _road(road)
        launches[road] = _launches(run)
    ms = _alternate(run, rounds, iters)
    return _row(ms, row='block', set=name, graphs=B, nmax=nmax, cin=Cin, c=C, bias=bias, dx=not first, launches_fused=launches['fused'],
                launches_composition=launches['composition'])


def _step(batch, rounds, iters, dev):
    from gnn_matlang_amd import models
    torch.manual_seed(0)
    m = models.zinc_ppgn().to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)

    def run():
        opt.zero_grad(set_to_none=True)
        models.zinc_loss(m(batch, _road='torch' if os.environ.get(ENV) else None), batch.y).backward()
        opt.step()
    return _row(_alternate(run, rounds, iters), row='step', set='zinc', graphs=batch.num_graphs, model='zinc_ppgn')


def _seed(name, batch, factory, pairs, rounds, iters, dev):
    from gnn_matlang_amd import expressivity
    out = {}

    def run():
        out['count'] = expressivity.count_similar(factory, batch, seeds=[0], pairs=pairs)[-1]
    row = _row(_alternate(run, rounds, iters, sync_host=True), row='seed', set=name, graphs=batch.num_graphs, model=factory.__name__)
    row['similar_after_seed0'] = out['count']
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ppgn.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_ppgn.py measures on the GPU: none found')
    from gnn_matlang_amd import expressivity, models
    dev = torch.device('cuda:0')
    sets = _sets(dev)
    _block('sr25', sets['sr25'], 32, True, True, 1, a.iters, dev)          # discarded: the first shape a process measures reads high
    rows = []
    for name, C, bias in (('sr25', 32, True), ('graph8c', 32, True), ('exp', 20, False), ('zinc', 32, False)):
        for first in (True, False):
            big = sets[name].X2.size(0) > 1000
            rows.append(_block(name, sets[name], C, first, bias, a.rounds, max(4, a.iters // 4) if big else a.iters, dev))
            print(json.dumps(rows[-1]), flush=True)
    rows.append(_step(sets['zinc'], a.rounds, a.iters, dev))
    print(json.dumps(rows[-1]), flush=True)
    for name, factory, pairs in (('sr25', models.sr25_ppgn, None), ('graph8c', models.graph8c_ppgn, None),
                                 ('exp', models.exp_ppgn, expressivity.exp_pairs(sets['exp'].num_graphs))):
        rows.append(_seed(name, sets[name], factory, pairs, a.rounds, max(3, a.iters // 5), dev))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(tool='tools/bench_ppgn.py', device=torch.cuda.get_device_name(0),
               what='ms; median of rounds x iters samples per road, roads alternating in one process; block and step: device-event '
                    'intervals; seed: host clock around count_similar(seeds=[0]), which ends in a host read',
               launches_per_block=dict(fused_forward=3, fused_backward_with_dx=5, fused_backward_without_dx=4),
               rounds=a.rounds, iters=a.iters, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
