"""freqclass.py's GNNML3 (three ML3Layer(learnedge=False, 64 + 2) over S = 6 supports, graphs of 200 nodes, batch 64) on its two roads:
the batched dense blocks (DeviceDataset.batch_dense -> csrc/gml_dense_mid.hip + tall GEMMs) and the sparse CSR kernels on the same
graphs collated with edges.  bandclass.mat is not available: the graphs are synthetic.make_graphs('bandclass', 64, n=200), and the mask
fill they have is recorded with the result.  Three measurements, device events, the roads alternating in ONE process, medians with the
10th / 90th percentiles:

  1. gml_dense_mid_support_mm alone, forward and adjoint at F = 66: time, image bytes, and its algorithmic bytes per second as a
     fraction of the rate of a plain device copy measured in the same process;
  2. one ML3Layer (66 -> 64 + 2) forward + backward, dense against sparse;
  3. the whole train step (forward, sum BCE, backward, OneLaunchAdam) eagerly on both roads, and as ONE captured step on the dense road.

    python tools/bench_freqclass.py [--rounds 5] [--iters 50] [--graphs 64] [--out profiles/freqclass_gnnml3.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_matlang_amd import DeviceDataset, SpectralDesign, collate, models, synthetic     # noqa: E402
from gnn_matlang_amd import dense_block as DB                                               # noqa: E402
from gnn_matlang_amd.dist import TrainStep                                                  # noqa: E402
from gnn_matlang_amd.optim import OneLaunchAdam                                             # noqa: E402


def timed(runs, rounds, iters):
    """runs: name -> callable.  Round 0 warms every road up; then `rounds` rounds, the roads alternating, `iters` device-event
    intervals each.  -> name -> dict(ms, p10_p90, samples)"""
    ms = {k: [] for k in runs}
    for rnd in range(rounds + 1):
        for name, run in runs.items():
            run()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
            ev[0].record()
            for i in range(iters):
                run()
                ev[i + 1].record()
            torch.cuda.synchronize()
            if rnd:
                ms[name] += [ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]
    return {k: dict(ms=round(statistics.median(v), 4), p10_p90=[round(statistics.quantiles(v, n=10)[i], 4) for i in (0, 8)], samples=len(v))
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--graphs', type=int, default=64)
    ap.add_argument('--nodes', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_freqclass.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    B, n = a.graphs, a.nodes
    ds = SpectralDesign(recfield=2, dv=4, nfreq=5).design_many(synthetic.make_graphs('bandclass', B, seed=0, n=n))
    fills = [d['edge_index2'].shape[1] / float(n * n) for d in ds]
    dd = DeviceDataset.from_graphs(ds, dev)
    bank = dd.equal_bank()
    ids = torch.arange(B, device=dev)
    dense, sparse = dd.batch_dense(ids), collate(ds).to(dev)
    S, KP, F = bank.S, bank.KP, 66
    res = dict(tool='tools/bench_freqclass.py', graphs=B, nodes=n, S=S, rounds=a.rounds, iters=a.iters,
               data="synthetic.make_graphs('bandclass', %d, seed=0, n=%d): a stand-in, bandclass.mat is not available" % (B, n),
               mask_fill=dict(min=round(min(fills), 4), mean=round(sum(fills) / B, 4), max=round(max(fills), 4)),
               mask_entries=int(sparse.edge_index2.size(1)))

    # ---- 1. the support product alone, against the device's own copy rate
    x = torch.randn(B * n, F, device=dev)
    gh = torch.randn(B * n, S * F, device=dev)
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev)        # 256 MB: well past the last-level cache
    dst = torch.empty_like(src)
    t = timed(dict(fwd=lambda: DB.support_mm(bank.fwd, x, bank, F, 0, F, False, dense.gid),
                   adj=lambda: DB.support_mm(bank.bwd, gh, bank, F, F, 0, True, dense.gid),
                   copy=lambda: dst.copy_(src)), a.rounds, a.iters)
    copy_rate = 2 * src.numel() * 4 / (t['copy']['ms'] * 1e-3)
    img_bytes = B * S * 2 * n * KP * 2
    for k, act_cols, out_cols in (('fwd', F, S * F), ('adj', S * F, F)):
        byts = img_bytes + 4 * B * n * (act_cols + out_cols)
        t[k].update(image_bytes=img_bytes, algorithmic_bytes=byts, bytes_per_s=round(byts / (t[k]['ms'] * 1e-3)),
                    fraction_of_copy_rate=round(byts / (t[k]['ms'] * 1e-3) / copy_rate, 4),
                    flops_bf16x3=3 * 2 * B * S * n * KP * F)
    t['copy'].update(bytes=2 * src.numel() * 4, bytes_per_s=round(copy_rate))
    res['support_product_F66'] = t
    print(json.dumps(dict(support_product_F66=t)), flush=True)
    del src, dst

    # ---- 2. one ML3Layer 66 -> 64 + 2, forward + backward
    torch.manual_seed(0)
    layer = models.GNNML3(F, S, 64, 2, 1, learnedge=False, pool=None, head='node').to(dev)
    xin = torch.randn(B * n, F, device=dev)
    gout = torch.randn(B * n, 66, device=dev)
    batches = {}
    for road, b in (('dense', dense), ('sparse', sparse)):
        fields = {k: v for k, v in b.__dict__.items() if not k.startswith('_')}
        fields['x'] = xin.clone().requires_grad_(True)
        batches[road] = type(b)(**fields)

    def layer_run(road):
        def run():
            for q in layer.parameters():
                q.grad = None
            batches[road].x.grad = None
            layer(batches[road], _features=True).backward(gout)
        return run
    t = timed(dict(dense=layer_run('dense'), sparse=layer_run('sparse')), a.rounds, a.iters)
    t['sparse_over_dense'] = round(t['sparse']['ms'] / t['dense']['ms'], 3)
    res['layer_66_to_64p2_fwd_bwd'] = t
    print(json.dumps(dict(layer_66_to_64p2_fwd_bwd=t)), flush=True)

    # ---- 3. the whole train step
    steps = {}
    for road, b in (('dense', dense), ('sparse', sparse), ('dense_captured', dd.batch_dense(ids))):
        torch.manual_seed(1)
        m = models.freqclass_gnnml3().to(dev).train()
        ts = TrainStep(m, models.freqclass_step_loss, OneLaunchAdam(m.parameters(), lr=1e-3))
        if road == 'dense_captured':
            replay, _ = ts.capture(b)
            steps[road] = replay
        else:
            steps[road] = (lambda ts=ts, b=b: ts.step(b))
    t = timed(steps, a.rounds, a.iters)
    t['sparse_over_dense'] = round(t['sparse']['ms'] / t['dense']['ms'], 3)
    t['sparse_over_dense_captured'] = round(t['sparse']['ms'] / t['dense_captured']['ms'], 3)
    res['train_step'] = t
    print(json.dumps(dict(train_step=t)), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
