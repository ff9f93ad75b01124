"""Fresh batches of any size: the ZINC GNNML3 train step at 131,072 graphs on a resident batch against a NEW exact batch every step
(DeviceDataset.batch_assembled(ids, None, sym=True): gml_batch_assemble_any + the data set's mirror pairing), the fresh-batch road of
bench.py (batch() gathers + GraphCSR.from_edge_index + the per-batch pairing pass), the assembly alone, and the captured batch-64
epoch with sym off and on.  Synthetic data: 512 designed ZINC-like graphs tiled to twice the batch.  Prints one JSON line per
measurement.

    python tools/bench_assembled.py [--batch 131072] [--steps 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def out(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=131072)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--ref-batch', type=int, default=64)
    args = ap.parse_args()
    from gnn_matlang_amd import SpectralDesign, functional as Fn, models, synthetic
    from gnn_matlang_amd.dataset import DeviceDataset
    from gnn_matlang_amd.optim import OneLaunchAdam
    dev = torch.device('cuda:0')
    raw = synthetic.make_graphs('zinc', 512, seed=1000)
    base = DeviceDataset.from_graphs(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw), dev)
    base.y = base.y.float()
    B = args.batch
    dd = base.tiled(max(2, -(-2 * B // len(base))))
    dd.prepare()
    pair = dd.pairing()
    out(what='data', graphs=len(dd), support_edges=int(dd.edge_index2.size(1)),
        unique_rows=None if pair is None else int(pair['uid'].numel()))
    G = len(dd)
    gen = torch.Generator().manual_seed(3)

    def fresh_ids():
        return torch.randperm(G, generator=gen)[:B].to(dev)

    torch.manual_seed(0)
    m = models.zinc_gnnml3().to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, fused=True)

    def step(b):
        opt.zero_grad(set_to_none=True)
        loss = models.zinc_step_loss(m, b)
        with Fn.deferred_folds(list(m.parameters())):
            loss.backward()
        opt.step()
        return loss

    def timed(fn, n, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    pool = [fresh_ids().contiguous() for _ in range(4)]     # (drawn before the timing: the host randperm is not the step's work)
    turn = [0]

    def next_ids():
        turn[0] += 1
        return pool[turn[0] % len(pool)]
    ids0 = fresh_ids()
    res = dd.batch_assembled(ids0, None)                   # = batch(ids) + GraphCSR.from_edge_index, built once
    t_res = timed(lambda: step(res), args.steps)
    out(what='resident', batch=B, ms_per_step=t_res, note='one exact batch built once (its pairing pass runs once and is cached)')
    t_fresh = timed(lambda: step(dd.batch_assembled(next_ids(), None, sym=True)), args.steps)
    out(what='fresh_exact_sym', batch=B, ms_per_step=t_fresh, ratio_vs_resident=t_fresh / t_res,
        note='a new exact batch every step: batch_assembled(ids, None, sym=True), two host reads per batch')
    t_road = timed(lambda: step(dd.batch(next_ids())), args.steps)
    out(what='fresh_batch_road', batch=B, ms_per_step=t_road, ratio_vs_resident=t_road / t_res,
        note='batch(ids) + GraphCSR.from_edge_index + the per-batch pairing pass (bench.py fresh_batch with new graphs)')

    def assemble_only(sym, exact=True):
        return dd.batch_assembled(next_ids(), None if exact else bd_big, sym=sym)
    bd_big = dd.bounds(B)
    for sym in (False, True):
        out(what='assembly_exact', sym=sym, batch=B, ms=timed(lambda: assemble_only(sym), args.steps))
        out(what='assembly_padded', sym=sym, batch=B, ms=timed(lambda: assemble_only(sym, exact=False), args.steps))
    del res

    # ---- the captured batch-64 epoch, sym off / on
    ep = base.tiled(20)
    ep.prepare()
    Bq = args.ref_batch
    bd = ep.bounds(Bq)
    Gq = len(ep)
    for sym in (False, True):
        torch.manual_seed(0)
        cm = models.zinc_gnnml3().to(dev)
        co = OneLaunchAdam(cm.parameters(), lr=1e-3)
        ids_buf = torch.arange(Bq, device=dev)
        loss_acc = torch.zeros((), device=dev)
        one = torch.ones((), device=dev)

        def padded_step():
            b = ep.batch_assembled(ids_buf, bd, sym=sym)
            co.zero_grad(set_to_none=True)
            l = models.zinc_step_loss(cm, b, loss_sum=loss_acc)
            with Fn.deferred_folds(list(cm.parameters())):
                l.backward(one)
            co.step()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                padded_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            padded_step()
        egen = torch.Generator().manual_seed(7)

        def epoch():
            perm = torch.randperm(Gq, generator=egen).to(dev)
            perm = torch.cat([perm, torch.full(((-Gq) % Bq,), Gq, dtype=torch.int64, device=dev)])
            for i in range(0, perm.numel(), Bq):
                ids_buf.copy_(perm[i:i + Bq])
                cg.replay()
            return perm.numel() // Bq
        epoch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nb = epoch()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out(what='captured_epoch', batch=Bq, sym=sym, graphs=Gq, ms_per_step=dt / nb * 1e3, steps=nb)
        del cg


if __name__ == '__main__':
    main()
