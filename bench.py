#!/usr/bin/env python3
"""bench.py -- GNNML3 training-step throughput on ZINC-12k-shaped synthetic graphs (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--batch GRAPHS_PER_GPU | --global-batch GRAPHS] [--dump-outputs DIR] [--full]

K is the number of timed steps.  --dump-outputs DIR writes what the last of them returned (loss, parameters, gradients) as
DIR/<name>.npy; the inputs and the initial parameters are seeded, so two builds run with the same arguments can be compared
output for output.

A plain run does only what the headline needs: it builds the batch, warms up, settles the GPU (--min-seconds), times the K
steps, writes --dump-outputs and prints the line.  --full adds every side measurement listed below.  The timed steps and
their outputs are the same either way: the side measurements run after them, except the parity check at the initial
parameters, which changes nothing the step reads.

A step = forward + L1-sum loss + backward + (N>1: one flat SUM all-reduce of the gradients) + Adam,
of the reference's ZINC GNNML3 (Zinc12k.py:310-371: 4 x ML3Layer 30+2, S = 8 supports, 25 input
features, add-pool, fc 32 -> 1, lr 1e-3) over one batch of synthetic ZINC-like graphs per GPU (weak
scaling: graphs per GPU fixed; --global-batch: strong scaling).  Inputs are resident in HBM before the
timed region.  Storage and accumulation are fp32; the products run as split pieces on the matrix cores: the forward
pass fp32-class (edge branch three bf16 pieces / six products, conv projection f16 hi/lo under power-of-two scales), the
backward on bf16 hi/lo (``value_bf16x3`` is the same step with bf16 hi/lo in the forward too -- rounds 1-5's headline
arithmetic, whose trained-state gradients miss 1e-4; ``value_exact_fp32`` the step with exact fp32 products everywhere).

With --gpus N > 1 and no WORLD_SIZE in the environment bench.py starts the N ranks itself
(python -m torch.distributed.run ...) before touching the GPU and relays rank 0's line.

Rank 0 prints ONE JSON line.  Besides the contract's fields, with --full (and the full record in bench_extras.json):
  roofline        the dominant kernel (fused SpectConv backward), timed live with HIP events on the launch stream
  fresh_batch     the same step when every step receives a NEW batch: CSR, group records, bf16 pre-split and the
                  source-order copy are rebuilt inside the timed region (the reference reshuffles every epoch)
  epoch_bs64      one shuffled epoch over 10,000 distinct graphs at the reference's batch size 64, batches assembled
                  on the device (gnn_matlang_amd.dataset), index build included, end to end
  ref_batch       one batch-64 step replayed from a HIP graph (launch-latency floor of that batch size)
  cpu_baseline    the CPU oracle (a port of the reference algorithm, op for op) on this box's host cores (N = 1 only)
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 measured achievable
MFMA_F32_PEAK_TFLOPS = 157.3  # dense f32-in MFMA (= fp32 vector) peak
DTYPE = 'f32 storage/accumulate; forward products fp32-class (edge branch bf16x6, conv f16x3 split), backward products bf16x3 split'


LINE_BUDGET = 6000           # characters: the driver's capture keeps only the tail of stdout (8,000 characters in round 5)


def _sig(v, digits=6):
    """Floats to `digits` significant figures (recursively): the line is a record, not a checkpoint."""
    if isinstance(v, float):
        return float('%.*g' % (digits, v)) if v == v and abs(v) != float('inf') else None
    if isinstance(v, dict):
        return {k: _sig(x, digits) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_sig(x, digits) for x in v]
    return v


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def compact_line(res):
    """The ONE JSON line of the contract, from the full result record: contract fields + config + dtype + roofline (dominant
    kernel, with traffic) + cpu_baseline + the handful of side figures VERDICT r05 names, every free-text field cut short.
    Everything else (other configs, sweeps, parity blocks, ladders, block lists) goes to bench_extras.json / stderr.
    Guaranteed json.loads-able and shorter than LINE_BUDGET characters (tests/test_host_cpu.py::test_bench_line_is_compact)."""
    cut = lambda s, n=96: s if not isinstance(s, str) or len(s) <= n else s[:n - 1] + '~'
    out = _pick(res, ['metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                      'vs_baseline', 'dtype', 'data'])
    if 'config' in res:
        c = dict(res['config'])
        c['workload'] = cut(c.get('workload'), 160)
        out['config'] = c
    if 'roofline' in res:
        r = _pick(res['roofline'], ['bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'kernel', 'launches', 'avg_launch_ms',
                                    'ms_per_step', 'algorithmic_bytes_per_launch', 'traffic_source'])
        r['kernel'] = cut(r.get('kernel'), 80)
        r['traffic_source'] = cut(r.get('traffic_source'), 80)
        out['roofline'] = r
    if 'cpu_baseline' in res:
        c = _pick(res['cpu_baseline'], ['value', 'unit', 'cores', 'kind', 'sample', 'ms_per_step', 'cpu_model', 'host_cores', 'spread'])
        c['sample'] = cut(c.get('sample'), 200)
        out['cpu_baseline'] = c
    for k in ('roofline_step', 'roofline_step_compulsory'):
        if k in res:
            out[k] = _pick(res[k], ['bound', 'algorithmic_bytes_per_step', 'achieved', 'peak', 'unit', 'frac'])
    if 'spmm' in res:
        out['spmm'] = _pick(res['spmm'], ['bound', 'achieved', 'peak', 'unit', 'frac', 'avg_launch_ms', 'algorithmic_bytes_per_launch', 'S', 'Fin'])
    if 'kernels_ms_per_step' in res:
        out['kernels_ms_per_step'] = res['kernels_ms_per_step']
    for k in ('value_exact_fp32', 'value_bf16x3', 'value_all_rows'):
        if k in res:
            out[k] = _pick(res[k], ['value', 'unit', 'ms_per_step'])
    for k in ('fresh_batch', 'distinct_graphs', 'ref_batch'):
        if k in res:
            out[k] = _pick(res[k], ['value', 'ms_per_step'])
    if 'epoch_bs64' in res:
        out['epoch_bs64'] = _pick(res['epoch_bs64'], ['value', 'unit', 'ms_per_step', 'graphs', 'batch_size'])
    for k in ('max_rel_err_vs_oracle', 'max_rel_err_vs_oracle_after_training'):
        if k in res:
            out[k] = res[k]
    for k in ('final_loss', 'blocks', 'n_ranks_seen', 'rccl_version', 'hbm_copy_GBps', 'per_rank_ms_per_step', 'extras'):
        if k in res:
            out[k] = res[k]
    if 'edge_unique_rows' in res:
        out['edge_unique_rows'] = _pick(res['edge_unique_rows'], ['share', 'enabled'])
    def cut_all(v, n=120):
        if isinstance(v, dict):
            return {k: cut_all(x, n) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [cut_all(x, n) for x in v[:16]]
        return cut(v, n)
    for k in ('sharding', 'data_parallel'):                      # N > 1 / --global-batch: per-rank cut and times, all-reduce cost
        if k in res:
            out[k] = cut_all(res[k])
    out = _sig(out)
    line = json.dumps(out, separators=(',', ':'))
    # never exceed the budget: drop the side figures, least important first (the contract fields, config, roofline and
    # cpu_baseline are never dropped)
    for k in ('per_rank_ms_per_step', 'max_rel_err_vs_oracle', 'data_parallel', 'sharding', 'kernels_ms_per_step', 'ref_batch', 'distinct_graphs', 'fresh_batch',
              'roofline_step', 'epoch_bs64', 'max_rel_err_vs_oracle_after_training', 'spmm', 'value_exact_fp32',
              'roofline_step_compulsory'):
        if len(line) <= LINE_BUDGET:
            break
        out.pop(k, None)
        line = json.dumps(out, separators=(',', ':'))
    assert len(line) <= LINE_BUDGET, len(line)
    return line


def write_extras(res):
    """The full record next to bench.py (and under gpurun_out/ when that exists: it is what comes back from the GPU box)."""
    paths = [os.path.join(ROOT, 'bench_extras.json')]
    if os.path.isdir(os.path.join(ROOT, 'gpurun_out')):
        paths.append(os.path.join(ROOT, 'gpurun_out', 'bench_extras.json'))
    done = []
    for p in paths:
        try:
            with open(p, 'w') as f:
                json.dump(res, f)
            done.append(p)
        except OSError:
            pass
    return done


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20, help='K: the number of timed steps')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=131072, help='graphs per GPU per step (SURVEY s8d: 65,536 .. 262,144 for the roofline run)')
    ap.add_argument('--global-batch', type=int, default=0, help='strong scaling: total graphs per step, split over the ranks')
    ap.add_argument('--pool', type=int, default=2048, help='distinct synthetic graphs (tiled to --batch)')
    ap.add_argument('--min-seconds', type=float, default=3.0, help='before the timed steps, keep the GPU busy this long with the same '
                    'step on a copy of the model (the timed steps and their outputs are the same whatever this is)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help='after the timed steps write what the last timed step '
                    'returned to its caller as DIR/<name>.npy: the loss, the parameters the step left and their gradients')
    ap.add_argument('--full', action='store_true', help='also take every side measurement: rooflines and '
                    'per-kernel times, other arithmetics, sizes and configs, the reference batch size, the CPU baseline, the parity '
                    'checks against the oracle, the data-parallel costs; writes the full record to bench_extras.json.  The '
                    'options below narrow a --full run; a plain run takes none of these measurements')
    ap.add_argument('--cpu-graphs', type=int, default=2048)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--no-profile', action='store_true', help='skip the live per-kernel HIP-event timing and the extra measurements')
    ap.add_argument('--no-extras', action='store_true', help='skip fresh_batch / epoch_bs64 / value_exact_fp32')
    ap.add_argument('--distinct', type=int, default=131072, help='extra measurement: the step over this many DISTINCT graphs '
                    '(no tiling of a pool), supports built by the device SpectralDesign; 0 = skip')
    ap.add_argument('--ref-batch', type=int, default=64, help='also time the reference batch size (Zinc12k.py:20) as a '
                    'HIP-graph-captured step; 0 = skip')
    args = ap.parse_args()
    if not args.full:                                  # a plain run: none of the side measurements
        args.no_cpu = args.no_profile = args.no_extras = True
        args.distinct = args.ref_batch = 0
    return args


def dump_outputs(out_dir, loss, model):
    """--dump-outputs: what one training step hands its caller -- the loss it returns, the parameters it leaves in the model and
    their gradients -- as out_dir/<name>.npy in float32 (loss.npy, param.<name>.npy, grad.<name>.npy).  The model is small
    (33,309 parameters): the whole of it is written, far below 64 MB.  Returns the bytes written."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {'loss': loss}
    for n, p in model.named_parameters():
        arrays['param.' + n] = p
        arrays['grad.' + n] = p.grad
    nbytes = 0
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        np.save(os.path.join(out_dir, name + '.npy'), a)
        nbytes += a.nbytes
    assert nbytes <= 64 << 20, nbytes
    return nbytes


def spawn_ranks(args):
    """--gpus N from a bare shell: start N fresh rank processes (never re-exec a process that touched the GPU)."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    r = subprocess.run(cmd, env=env)
    sys.exit(r.returncode)


def build_batch(graphs_per_gpu, pool, seed, device):
    """pool distinct ZINC-like graphs -> supports -> tiled on the device to graphs_per_gpu graphs."""
    import torch
    from gnn_matlang_amd import SpectralDesign, collate, synthetic
    from gnn_matlang_amd.graph import Batch
    pool = min(pool, graphs_per_gpu)
    raw = synthetic.make_graphs('zinc', pool, seed=seed)
    ds = SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw)      # Zinc12k.py:12
    base = collate(ds).to(device)
    reps = (graphs_per_gpu + pool - 1) // pool
    n, B = base.x.size(0), base.num_graphs
    offs = (torch.arange(reps, device=device) * n)
    x = base.x.repeat(reps, 1)
    ei2 = (base.edge_index2.unsqueeze(1) + offs.view(1, -1, 1)).reshape(2, -1)
    ei = (base.edge_index.unsqueeze(1) + offs.view(1, -1, 1)).reshape(2, -1)
    ea = base.edge_attr2.repeat(reps, 1)
    batch = (base.batch.unsqueeze(0) + (torch.arange(reps, device=device) * B).view(-1, 1)).reshape(-1)
    ptr = (base.ptr[:-1].long().view(1, -1) + offs.view(-1, 1)).reshape(-1)
    ptr = torch.cat([ptr, torch.tensor([n * reps], device=device)])
    g = torch.Generator(device='cpu').manual_seed(seed)
    y = torch.randn(B * reps, generator=g).to(device)
    full = Batch(x=x, edge_index=ei, edge_index2=ei2, edge_attr2=ea, batch=batch, ptr=ptr.int(), y=y)
    return full, base


def build_batch_distinct(graphs, seed, device):
    """`graphs` DISTINCT ZINC-like graphs (no tiling): generated on the host, supports by the device SpectralDesign
    (gnn_matlang_amd.spectral_design.design_device, libs/utils.py:546-610 on the GPU)."""
    import torch
    from gnn_matlang_amd import SpectralDesign, collate, synthetic
    from gnn_matlang_amd.graph import Batch
    raw = synthetic.make_graphs('zinc', graphs, seed=seed)
    host = collate([dict(x=g[0], edge_index=g[1], y=g[2]) for g in raw])
    x, ei, ptr = host.x.to(device), host.edge_index.to(device), host.ptr.to(device)
    d = SpectralDesign(recfield=2, dv=2, nfreq=7).design_device(x, ei, ptr)
    return Batch(x=d['x'], edge_index=ei, edge_index2=d['edge_index2'], edge_attr2=d['edge_attr2'], batch=host.batch.to(device),
                 ptr=ptr.int(), y=host.y.float().to(device))


def cpu_model_name():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def cpu_oracle_rate(host_batch, nsteps, warm, threads):
    """the oracle (port of the reference CPU algorithm) on the host cores: median step time of fwd + bwd + Adam"""
    import torch
    from oracle import models_oracle as MO
    torch.set_num_threads(threads)
    b = host_batch
    torch.manual_seed(0)
    m = MO.zinc_gnnml3(25, 8)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    B = b.num_graphs

    def step():
        opt.zero_grad()
        l = MO.zinc_loss(m(b.x, b.edge_index2, b.edge_attr2, b.batch, B), b.y)
        l.backward()
        opt.step()
    for _ in range(warm):
        step()
    t = []
    for _ in range(nsteps):
        t0 = time.perf_counter()
        step()
        t.append(time.perf_counter() - t0)
    med = float(np.median(t))
    return dict(value=B / med, unit='graphs/s', threads=torch.get_num_threads(), graphs_per_step=B,
                nodes=int(b.x.size(0)), support_edges=int(b.edge_index2.size(1)), warmup=warm, timed_steps=nsteps,
                ms_per_step=med * 1e3, min_ms=float(np.min(t)) * 1e3, max_ms=float(np.max(t)) * 1e3)


def parity_vs_oracle(model, data, base, log):
    """one forward + backward of the bench's own batch in each arithmetic mode against the float64 oracle (checker leg)."""
    import torch
    from gnn_matlang_amd import functional as Fn, models
    from oracle import parity_at_size as PS
    host = base.to(torch.device('cpu'))
    torch.cuda.synchronize()
    out = dict(graphs=int(data.num_graphs), pool_graphs=int(base.num_graphs), tolerance=1e-4,
               criterion='|got - ref| <= 1e-4 * T per element; T = sum of |terms| at product level, per layer from the float64 activations and output gradients (oracle/parity_at_size.py, oracle/termsums.py), ref = oracle in float64',
               modes={})
    T = None
    for mode in ('default', 'bf16x3', 'f32'):
        for p_ in model.parameters():
            p_.grad = None
        outs, n0_ = {}, int(base.x.size(0))
        hooks = [getattr(model, 'conv%d' % i).register_forward_hook(lambda mod, inp, o, i=i: outs.__setitem__(i, o.detach()))
                 for i in range(1, model.nlayers)]
        keep = Fn.EDGE_FWD6, Fn.FWD_F16
        if mode == 'bf16x3':                               # bf16 hi/lo pieces in the forward too (rounds 1-5's default)
            Fn.EDGE_FWD6 = Fn.FWD_F16 = False
        try:
            with Fn.exact_products(mode == 'f32'):
                cap = {}
                pre = model(data, _capture=cap)
                models.zinc_loss(pre, data.y).backward()
                for h_ in hooks:
                    h_.remove()
                with torch.no_grad():                      # the last layer's per-node output (inside the model it is pooled in its own
                    L_ = model.nlayers                     # autograd node): the same kernels on the same input -- the same values
                    outs[L_] = getattr(model, 'conv%d' % L_)(outs[L_ - 1], data.csr('edge_index2'), data.edge_attr2)
        finally:
            Fn.EDGE_FWD6, Fn.FWD_F16 = keep
        outs = {i: o[:n0_].clone() for i, o in outs.items()}      # first copy (the copies are bit-identical on the device: tools/parity_diag.py)
        grads_dev = {n: p_.grad.detach().cpu().numpy() for n, p_ in model.named_parameters()}
        ref = PS.reference(host, model.state_dict(), data.y, pre_dev=pre[:, 0], T=T, head_pre_dev=cap['head_pre'])
        flips = PS.relu_mask_diffs(host, model.state_dict(), data.y, pre[:, 0], outs)
        T = ref['T']
        rep = PS.compare(ref, pre[:, 0].detach().cpu().numpy(), grads_dev)
        # the same with the float64 pass evaluated on the DEVICE's activation pattern of every layer's relu(conv) columns: the gradients
        # given the forward's discrete decisions
        c1s = {i: int(getattr(model, 'conv%d' % i).conv1.weight.size(2)) for i in outs}
        ref_m = PS.reference(host, model.state_dict(), data.y, pre_dev=pre[:, 0], T=T, head_pre_dev=cap['head_pre'],
                             layer_masks_dev={i: o[:, :c1s[i]] > 0 for i, o in outs.items()})
        rep_m = PS.compare(ref_m, pre[:, 0].detach().cpu().numpy(), grads_dev)
        worst = max(rep['tensors'].items(), key=lambda kv: kv[1]['termsum'])
        out['modes'][mode] = dict(logits_rel_err=rep['logits_rel_err'], max_rel_err_termsum=rep['worst_termsum'],
                                  max_rel_err_maxnorm=rep['worst_maxnorm'], worst_tensor=worst[0], ok=rep['ok'],
                                  max_rel_err_termsum_on_the_device_activation_pattern=rep_m['worst_termsum'], ok_on_the_device_activation_pattern=rep_m['ok'],
                                  head_units_flipped=ref['head_units_flipped'], relu_units_on_the_other_side_of_zero=flips,
                                  oracle_seconds=round(ref['seconds'], 2))
        nflip = sum(v['differing'] for v in flips.values())
        log('parity at bench size, %s: logits %.2e, gradients %.2e of their term sums (worst: %s), %s; %d of %d relu units on the other side of zero' % (
            mode, rep['logits_rel_err'], rep['worst_termsum'], worst[0], 'within 1e-4' if rep['ok'] else 'beyond 1e-4 (forward error of the bf16 pairs: relu units downstream decide differently, DESIGN s6)',
            nflip, sum(v['units'] for v in flips.values())) + '; with the float64 pass on the device\'s activation pattern: %.2e' % rep_m['worst_termsum'])
        wm = max(rep_m['tensors'].items(), key=lambda kv: kv[1]['termsum'])
        log('   worst element on the device pattern: %s%s got %.6e ref %.6e T %.3e (tensor max %.3e)' % (wm[0], wm[1]['worst_index'], wm[1]['worst_got'], wm[1]['worst_ref'], wm[1]['worst_T'], wm[1]['tensor_max_abs']))
    # the reference arithmetic itself under the same criterion: the oracle in float32 on the CPU (what "fp32-class" means here)
    try:
        pre32, g32, z32 = PS.oracle_fp32_as_device(host, model.state_dict(), data.y, pre[:, 0])
        ref = PS.reference(host, model.state_dict(), data.y, pre_dev=pre[:, 0], T=T, head_pre_dev=z32)
        rep = PS.compare(ref, pre32, g32)
        worst = max(rep['tensors'].items(), key=lambda kv: kv[1]['termsum'])
        out['modes']['reference_fp32_cpu'] = dict(logits_rel_err=rep['logits_rel_err'], max_rel_err_termsum=rep['worst_termsum'],
                                                  max_rel_err_maxnorm=rep['worst_maxnorm'], worst_tensor=worst[0], ok=rep['ok'],
                                                  note='the oracle (op-for-op port of the reference) in float32 on the host, same pool, same signs')
        log('parity at bench size, the reference arithmetic (oracle fp32 on the CPU): logits %.2e, gradients %.2e of their term sums' % (
            rep['logits_rel_err'], rep['worst_termsum']))
    except Exception as e:                                   # (never let the context line break the bench)
        out['modes']['reference_fp32_cpu'] = dict(error=repr(e))
    for p_ in model.parameters():
        p_.grad = None
    return out


def cpu_baseline(cpu_graphs, log):
    """the oracle at the reference batch size (64) and at a large batch, >= 5 warm-up + >= 20 timed steps,
    median; the thread count is chosen by a short ladder up to os.cpu_count() (ATen's intra-op threading of these
    small index ops stops scaling long before this box's core count)."""
    import torch
    from gnn_matlang_amd import SpectralDesign, collate, synthetic
    raw = synthetic.make_graphs('zinc', cpu_graphs, seed=1000)
    ds = SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw)
    host, host64 = collate(ds), collate(ds[:64])
    ncpu = os.cpu_count() or 1
    default_threads = torch.get_num_threads()
    ladder, best, worse = [], None, 0
    for th in [t for t in (8, 16, 32, 64, 128, 256) if t <= ncpu] or [ncpu]:
        r = cpu_oracle_rate(host, 2, 1, th)
        ladder.append(dict(threads=th, value=r['value']))
        log('cpu baseline ladder: %d graphs on %d threads -> %.0f graphs/s' % (host.num_graphs, th, r['value']))
        if best is None or r['value'] > best[1]:
            best, worse = (th, r['value']), 0
        else:
            worse += 1
            if worse >= 2:
                break
    th = best[0]
    large = cpu_oracle_rate(host, 20, 5, th)
    log('cpu baseline large: %.0f graphs/s (%d threads)' % (large['value'], th))
    bs64 = max((cpu_oracle_rate(host64, 20, 5, t) for t in sorted({min(8, ncpu), min(th, 16)})), key=lambda r: r['value'])
    log('cpu baseline bs64: %.0f graphs/s (%d threads)' % (bs64['value'], bs64['threads']))
    return dict(value=large['value'], unit='graphs/s', cores=large['threads'], kind='port',
                sample='%d ZINC-like graphs/step (N=%d, E=%d), %d timed steps after %d warm-up, median; fwd+bwd+Adam of '
                       'the oracle (op-for-op port of the reference CPU algorithm), torch CPU fp32'
                       % (large['graphs_per_step'], large['nodes'], large['support_edges'], large['timed_steps'], large['warmup']),
                ms_per_step=large['ms_per_step'], spread=dict(min_ms=large.get('min_ms'), max_ms=large.get('max_ms'), note='fastest / slowest of the timed steps (median reported): a shared host, the figure is context, not a ratio to quote'),
                large=large, bs64=bs64, thread_ladder=ladder,
                host_cores=ncpu, cpu_model=cpu_model_name(), torch_threads_default=default_threads)


_T0 = time.perf_counter()


def log(*a):
    if int(os.environ.get('RANK', '0')) == 0:
        print('[bench %7.1fs]' % (time.perf_counter() - _T0), *a, file=sys.stderr, flush=True)


def main():
    args = parse_args()
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        spawn_ranks(args)                                  # (before any GPU call)

    import torch
    import torch.distributed as dist
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world != args.gpus:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d' % (args.gpus, world))
    assert torch.cuda.is_available(), 'bench.py needs the MI355X (no CPU fallback)'
    # GML_BENCH_SHARE_DEVICE=1 (tests on a 1-GPU box): every rank on cuda:0 over gloo -- the N > 1 code path without RCCL
    share = os.environ.get('GML_BENCH_SHARE_DEVICE') == '1'
    if share:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    if world > 1:
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        if share:
            dist.init_process_group('gloo', rank=rank, world_size=world)
        else:
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)

    from gnn_matlang_amd import functional as Fn, models
    from gnn_matlang_amd.dist import FlatGradSync, broadcast_parameters
    from gnn_matlang_amd.graph import Batch

    per_gpu = args.batch
    scaling = 'weak'
    shard_info = None
    log('building data')
    if args.global_batch:
        # strong scaling: ONE global data set (the same on every rank: same seed), cut into contiguous ranges of equal
        # total support edges (graph.shard_graphs_balanced), each rank keeps its range
        from gnn_matlang_amd.graph import shard_graphs_balanced
        from gnn_matlang_amd.dataset import DeviceDataset
        scaling = 'strong'
        full, _ = build_batch(args.global_batch, args.pool, seed=1000, device=dev)
        B_ = full.num_graphs
        e2g = full.batch[full.edge_index2[0]]                                  # graph of every support edge
        work = torch.bincount(e2g, minlength=B_).cpu().numpy()
        lo, hi = shard_graphs_balanced(work, rank, world)
        nlo, nhi = int(full.ptr[lo]), int(full.ptr[hi])
        esel = (e2g >= lo) & (e2g < hi)
        esel1 = (full.batch[full.edge_index[0]] >= lo) & (full.batch[full.edge_index[0]] < hi)
        data = Batch(x=full.x[nlo:nhi].contiguous(), edge_index=full.edge_index[:, esel1] - nlo,
                     edge_index2=full.edge_index2[:, esel] - nlo, edge_attr2=full.edge_attr2[esel].contiguous(),
                     batch=full.batch[nlo:nhi] - lo, ptr=(full.ptr[lo:hi + 1] - nlo).int(), y=full.y[lo:hi].contiguous())
        shard_info = dict(graphs=hi - lo, support_edges=int(esel.sum()), global_support_edges=int(work.sum()))
        base = None
        del full, e2g, esel, esel1
    else:
        data, base = build_batch(per_gpu, args.pool, seed=1000 + rank, device=dev)
    log('data ready: %d graphs, %d nodes, %d support edges' % (data.num_graphs, data.x.size(0), data.edge_index2.size(1)))
    data.csr('edge_index2')                            # built once per batch (data loading, not the step); see fresh_batch
    torch.manual_seed(0)
    model = models.zinc_gnnml3().to(dev)
    broadcast_parameters(model)
    sync = FlatGradSync(model.parameters())
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)    # same update rule (Zinc12k.py:349), one multi-tensor kernel
    parity0 = None
    if world == 1 and not args.no_cpu and base is not None and data.num_graphs % base.num_graphs == 0:
        log('parity check at the initial parameters')
        parity0 = parity_vs_oracle(model, data, base, log)
        parity0['state'] = 'initial parameters (seed 0)'

    # the framework's own training step (dist.TrainStep): zero -> forward + L1-sum loss -> backward with the weight-gradient folds deferred
    # into ONE launch (functional.deferred_folds: bit-identical sums) -> flat all-reduce (nothing with one rank) -> fused Adam
    from gnn_matlang_amd.dist import TrainStep
    # (zinc_step_loss = zinc_loss(model(data), data.y) with the readout head + loss as one pass each way: functional.HeadL1BigFunction)
    trainer = TrainStep(model, lambda mod, d_: models.zinc_step_loss(mod, d_), opt, sync=sync)

    def step(d=None):
        return trainer.step(data if d is None else d)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_block(fn, nsteps):
        fence()
        t0 = time.perf_counter()
        for _ in range(nsteps):
            out = fn()
        fence()
        return time.perf_counter() - t0, out

    for _ in range(args.warmup):
        step()
    fence()
    log('warm-up done')
    def settle():
        """--min-seconds: keep the GPU busy that long right before the timed steps (so that a sampler sees it busy, and the timed
        steps run at the steady-state rate) with the same step on a COPY of the model and optimizer.  The copy is dropped: the timed steps
        start from the model the warm-up left, so what they compute does not depend on how many settling steps the clock allowed.
        (all ranks take the same number of blocks: rank 0's clock decides)"""
        import copy
        twin = copy.deepcopy(model)
        twin_trainer = TrainStep(twin, lambda mod, d_: models.zinc_step_loss(mod, d_), torch.optim.Adam(twin.parameters(), lr=1e-3, fused=True),
                                 sync=FlatGradSync(twin.parameters()))
        busy = 0.0
        while True:
            busy += timed_block(lambda: twin_trainer.step(data), args.steps)[0]
            more = busy < args.min_seconds
            if world > 1:
                flag = torch.tensor([1 if more else 0], device=dev)
                dist.broadcast(flag, 0)
                more = bool(flag.item())
            if not more:
                return busy

    # EXACTLY K timed steps, bracketed by barrier + synchronize.  Kernel events come from one more K-step block after them.
    # (the cyclic garbage collector is parked first, as timeit does: a collection is a host stall that leaves the GPU idle -- a
    #  full one between the settling and the timed steps made the 20 timed steps ~1.5 % slower; a generation-2 pass (~65 ms)
    #  in the block that records two HIP events per launch shows up as GPU idle time inside one event pair)
    import gc
    gc.collect()
    gc.disable()
    try:
        if args.min_seconds > 0:
            log('settled: %.2f s of steps on a copy of the model' % settle())
        own_dt, loss = timed_block(step, args.steps)
        if args.dump_outputs and rank == 0:
            nbytes = dump_outputs(args.dump_outputs, loss, model)
            log('outputs of the last timed step: %.1f KB in %s' % (nbytes / 1024, args.dump_outputs))
        if not args.no_profile:
            Fn.PROFILE = {}
            timed_block(step, args.steps)
    finally:
        gc.enable()
    prof, Fn.PROFILE = Fn.PROFILE, None
    if os.environ.get('GML_BENCH_DUMP') and prof:            # debugging aid: per-launch HIP-event times of the profiled block
        for tag, recs in prof.items():
            ms = [r_[0].elapsed_time(r_[1]) for r_ in recs]
            n = max(len(ms) // args.steps, 1)
            log('launches of %s: %s' % (tag, [round(sum(ms[i::n]) / args.steps, 3) for i in range(n)]))
            log('   first launch of every step: %s' % [round(v, 2) for v in ms[0::n]])
    log('timed region: %d steps, %.3f s' % (args.steps, own_dt))
    tt = torch.tensor([own_dt], dtype=torch.float64, device=dev)
    gcount = torch.tensor([data.num_graphs], dtype=torch.int64, device=dev)
    if world > 1:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dist.all_reduce(gcount, op=dist.ReduceOp.SUM)
    dt = float(tt.item())
    graphs = int(gcount.item())
    shard_imb = None
    if shard_info is not None:                             # strong scaling: how even the cut by support edges came out
        se = torch.tensor([shard_info['support_edges'], shard_info['graphs']], dtype=torch.int64, device=dev)
        allse = [torch.zeros_like(se) for _ in range(world)]
        if world > 1:
            dist.all_gather(allse, se)
        else:
            allse = [se]
        edges = [int(t[0]) for t in allse]
        shard_imb = dict(method='graph.shard_graphs_balanced (contiguous ranges of equal total support edges)',
                         support_edges_per_rank=edges, graphs_per_rank=[int(t[1]) for t in allse],
                         max_over_mean=max(edges) / (sum(edges) / len(edges)))
    lossv = float(loss.item())
    assert np.isfinite(lossv) or os.environ.get('GML_BENCH_NOCHECK'), 'loss diverged'   # (NOCHECK: ablation builds)
    dp = None
    if world > 1 and args.full:
        # ---- what the collective costs (every rank runs this: collectives): each rank's own timed steps, the flat gradient
        #      all-reduce alone, and the reference's batch size per rank as ONE captured HIP graph with the all-reduce inside
        from gnn_matlang_amd.dist import TrainStep
        own = torch.tensor([own_dt / args.steps * 1e3], dtype=torch.float64, device=dev)
        per_rank = [torch.zeros_like(own) for _ in range(world)]
        dist.all_gather(per_rank, own)
        nparam = sum(p.numel() for p in model.parameters())
        flat = torch.zeros(nparam, dtype=torch.float32, device=dev)
        for _ in range(5):
            dist.all_reduce(flat)
        fence()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            dist.all_reduce(flat)
        e1.record()
        torch.cuda.synchronize()
        ar_ms = torch.tensor([e0.elapsed_time(e1) / 50], dtype=torch.float64, device=dev)
        dist.all_reduce(ar_ms, op=dist.ReduceOp.MAX)
        dp = dict(per_rank_ms_per_step=[float(t.item()) for t in per_rank], allreduce_ms=float(ar_ms.item()), allreduce_bytes=4 * nparam,
                  allreduce='ONE flat fp32 SUM all-reduce per step (dist.FlatGradSync), RCCL')
        try:
            rb64, _ = build_batch(64, 64, seed=7 + rank, device=dev)
            rb64.csr('edge_index2')
            torch.manual_seed(0)
            m64 = models.zinc_gnnml3().to(dev)
            broadcast_parameters(m64)
            from gnn_matlang_amd.optim import OneLaunchAdam      # Adam as ONE launch (gml_adam_many), step count on the device
            ts = TrainStep(m64, lambda mod, d_: models.zinc_step_loss(mod, d_), OneLaunchAdam(m64.parameters(), lr=1e-3))
            replay, gl64 = ts.capture(rb64)
            for _ in range(20):
                replay()
            fence()
            t64 = time.perf_counter()
            for _ in range(200):
                replay()
            fence()
            t64 = torch.tensor([(time.perf_counter() - t64) / 200 * 1e3], dtype=torch.float64, device=dev)
            dist.all_reduce(t64, op=dist.ReduceOp.MAX)
            dp['captured_bs64_per_rank'] = dict(ms_per_step=float(t64.item()), value=64 * world / (float(t64.item()) * 1e-3), unit='graphs/s',
                                                order=ts.order, mode='batch 64 per rank: forward + loss + backward + fold + flat all-reduce + fused '
                                                'Adam replayed from ONE HIP graph per rank (the collective is a graph node)')
        except Exception as e:                                 # noqa: BLE001  (recorded, not fatal: the eager path above is the measured one)
            dp['captured_bs64_per_rank'] = dict(error=repr(e)[:300])

    if rank == 0:
        ms = dt / args.steps * 1e3
        res = dict(metric='GNNML3 training graphs/sec on ZINC-12k', value=graphs * args.steps / dt, unit='graphs/s',
                   n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=ms, higher_is_better=True,
                   scaling=scaling, vs_baseline=None, dtype=DTYPE, data='synthetic',
                   config=dict(workload='Zinc12k.py GNNML3 regression train step (4x ML3Layer 30+2, S=8 supports, '
                                        'learnedge, add-pool, L1-sum, Adam 1e-3), ZINC-like synthetic graphs',
                               graphs_per_gpu=data.num_graphs, global_batch=graphs, nodes_per_gpu=int(data.x.size(0)),
                               support_edges_per_gpu=int(data.edge_index2.size(1)), supports=8,
                               parallelism='dp%d' % world, params=sum(p.numel() for p in model.parameters())),
                   final_loss=lossv, blocks=1, block_seconds=[round(own_dt, 4)],
                   n_ranks_seen=dist.get_world_size() if world > 1 else 1,
                   rccl_version='.'.join(str(v) for v in torch.cuda.nccl.version()) if (world > 1 and not share) else None)
        if args.full:
            try:                                               # share of the support rows the edge branch evaluates (the rest: bitwise mirrors)
                csr_ = data.csr('edge_index2')
                sym_ = csr_.sym_index(data.edge_attr2) if (Fn.EDGE_SYM and csr_.src_sorted) else None
                res['edge_unique_rows'] = dict(share=(sym_[0].numel() / csr_.E) if sym_ is not None else 1.0, enabled=bool(Fn.EDGE_SYM),
                                               note='edge (i, j) and its mirror (j, i) carry bitwise the same supports (symmetric spectral matrices): the edge '
                                                    'branch runs once per unique row, exact (csrc/gml_edge_chain_sym_impl.h); GML_EDGE_SYM=0 evaluates every row')
            except Exception as e_:                            # noqa: BLE001 (a context figure: never fatal)
                res['edge_unique_rows'] = dict(error=repr(e_)[:200])
        if shard_imb is not None:
            res['sharding'] = shard_imb
        if dp is not None:
            res['data_parallel'] = dp
        def rooflines(prof_):
            """(dominant kernel's roofline record, the other candidates, per-tag ms per step) of one profiled block"""
            summ = Fn.profile_summary(prof_)
            bf16x3 = not Fn.F32_MFMA
            BF16_PEAK_TFLOPS = 2500.0                       # dense bf16 MFMA (MI355X_MICROARCH.md)

            def roof(tag, kernel, proj_flops, edge_flops):
                """binding roof of one launch: HBM (algorithmic bytes), matrix pipe (projection flops: f32-input MFMA
                at 157.3 TF, or 3 bf16 MFMAs per product at 2.5 PF in the default bf16x3 arithmetic) or -- never
                binding here -- the fp32 VALU edge flops; achieved/peak are quoted for the binding one."""
                k = summ[tag]
                t = k['ms'] * 1e-3
                nl = k['launches']
                pf, ef = proj_flops / nl, edge_flops / nl
                gbs = k['bytes'] / t / 1e9
                t_hbm = k['bytes'] / (HBM_PEAK_GBS * 1e9)
                if bf16x3:
                    t_mat, mat_peak, mat_flops = 3 * pf / (BF16_PEAK_TFLOPS * 1e12), BF16_PEAK_TFLOPS, 3 * pf
                else:
                    t_mat, mat_peak, mat_flops = (pf + ef) / (MFMA_F32_PEAK_TFLOPS * 1e12), MFMA_F32_PEAK_TFLOPS, pf + ef
                if t_mat > t_hbm:
                    r = dict(bound='mfma', achieved=mat_flops / t / 1e12, peak=mat_peak, unit='TFLOP/s',
                             frac=mat_flops / t / 1e12 / mat_peak)
                else:
                    r = dict(bound='hbm', achieved=gbs, peak=HBM_PEAK_GBS, unit='GB/s', frac=gbs / HBM_PEAK_GBS)
                r.update(traffic=None, kernel=kernel, launches=nl, avg_launch_ms=k['ms'],
                         ms_per_step=k['ms'] * nl / args.steps,
                         projection_arith=(('f16 (hi, lo) split under power-of-two scales, 3 products on the f16 matrix cores, fp32 accumulate'
                                            if (tag == 'spectconv_fwd' and Fn.FWD_F16) else
                                            'bf16x3 split on the bf16 matrix cores, fp32 accumulate') if bf16x3 else 'f32-input MFMA'),
                         algorithmic_bytes_per_launch=k['bytes'], algorithmic_flops_per_launch=k['flops'],
                         t_hbm_ms=t_hbm * 1e3, t_matrix_ms=t_mat * 1e3, t_valu_edge_ms=ef / (MFMA_F32_PEAK_TFLOPS * 1e12) * 1e3,
                         hbm_GBps=gbs, hbm_frac=gbs / HBM_PEAK_GBS,
                         algorithmic_TFLOPs=k['flops'] / t / 1e12)
                return r
            # per-step flop split of the 4 layers (Fin = 25, 32, 32, 32; Fout = 30; S = 8): projections vs edge FMAs
            N_, E_ = int(data.x.size(0)), int(data.edge_index2.size(1))
            fins = [25, 32, 32, 32]
            pj_f = sum(2 * N_ * 8 * f * 30 for f in fins) * args.steps
            ed_f = sum(2 * E_ * 8 * f for f in fins) * args.steps
            pj_b = sum(6 * N_ * 8 * f * 30 for f in fins) * args.steps          # Z, dX, dW
            ed_b = sum(4 * E_ * 8 * 30 for f in fins) * args.steps              # P update + Z.g dot
            cands = []
            if 'spectconv_bwd' in summ:
                cands.append(roof('spectconv_bwd', '%s (fused SpectConv backward: dX, dval, dW%s)' % (
                    'gml_k_spectconv_bwd (f32-input MFMA)' if Fn.F32_MFMA else ('gml_k_spectconv_bwd4' if Fn.BWD_DMA else 'gml_k_spectconv_bwd3'),
                    '; carries the ML3Layer output stage' if (Fn.BWD_HAD and not Fn.F32_MFMA and not Fn.BWD_DMA) else ''), pj_b, ed_b))
            if 'spectconv_fwd' in summ:
                cands.append(roof('spectconv_fwd', '%s (fused SpectConv forward; also carries the Hadamard branch)' % ('gml_k_spectconv_fwd (f32-input MFMA)' if Fn.F32_MFMA else 'gml_k_spectconv_fwd3 (LDS-DMA ring)'), pj_f, ed_f))
            # HBM bytes per launch from the PMC counters: collected OFFLINE with the same command under rocprofv3
            # (separate FETCH_SIZE / WRITE_SIZE passes, gfx950 correction applied); valid for the code state and
            # workload the profile names -- the file records the commit it was taken at
            tpath = os.path.join(ROOT, 'profiles', 'hbm_traffic_b%d.json' % data.num_graphs)
            if os.path.exists(tpath) and args.pool == 2048 and bf16x3:
                tj = json.load(open(tpath))
                for r in cands:
                    pref = 'gml_k_spectconv_bwd' if 'backward' in r['kernel'] else 'gml_k_spectconv_fwd'
                    hits = [v for kname, v in tj['kernels'].items() if kname.startswith(pref)]
                    if hits:                                  # launch-weighted mean over the instantiations used
                        r['traffic'] = sum(h['hbm_bytes_per_launch'] * h.get('launches', 1) for h in hits) / \
                            sum(h.get('launches', 1) for h in hits)
                        r['traffic_source'] = 'profiles/%s: rocprofv3 PMC, per launch, measured OFFLINE at commit %s' % (
                            os.path.basename(tpath), tj.get('commit', '?'))
            cands.sort(key=lambda r: -r['ms_per_step'])          # first: the kernel with the largest share of the step
            return cands, {tag: round(v['ms'] * v['launches'] / args.steps, 4) for tag, v in summ.items()}
        if prof:
            cands, kms = rooflines(prof)
            res['roofline'] = cands[0]
            res['roofline_other'] = cands[1:]
            res['kernels_ms_per_step'] = kms
            # the whole step by the same accounting: sum of the SURVEY s8(d) algorithmic bytes of every tagged launch of a step / step time
            summ_ = Fn.profile_summary(prof)
            qstep = sum(v['bytes'] * v['launches'] for v in summ_.values()) / args.steps
            res['roofline_step'] = dict(bound='hbm', algorithmic_bytes_per_step=qstep, ms_per_step=ms,
                                        achieved=qstep / (ms * 1e-3) / 1e9, peak=HBM_PEAK_GBS, unit='GB/s',
                                        frac=qstep / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS)
            # the same step against its COMPULSORY bytes: SURVEY s8(d)'s fusion-agnostic Q_fwd + Q_bwd of the four
            # SpectConv layers alone -- what a step would move if the edge branch's output never touched HBM (it is written once and
            # re-read by each conv forward / backward and by the edge backward today) and pooling, head, loss and Adam were free
            csr_ = data.csr('edge_index2')
            S_c, widths = int(data.edge_attr2.size(1)), [(int(data.x.size(1)), 30)] + [(32, 30)] * 3      # Zinc12k.py:323-329
            qc = sum(Fn.conv_cost(csr_.N, csr_.E, S_c, fi, fo)[0] + Fn.conv_cost_bwd(csr_.N, csr_.E, S_c, fi, fo, need_x=li > 0)[0]
                     for li, (fi, fo) in enumerate(widths))
            res['roofline_step_compulsory'] = dict(bound='hbm', algorithmic_bytes_per_step=qc, ms_per_step=ms,
                                                   achieved=qc / (ms * 1e-3) / 1e9, peak=HBM_PEAK_GBS, unit='GB/s',
                                                   frac=qc / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                                   note='sum over the 4 layers of SURVEY s8(d) Q_fwd + Q_bwd (fusion-agnostic: no ea\' traffic)')
            log('roofline: dominant kernel %s at %.3f of the HBM roof (%.3f ms/launch); whole step %.3f (launched bytes), %.3f (compulsory bytes)' % (
                cands[0]['kernel'].split(' ')[0], cands[0]['frac'], cands[0]['avg_launch_ms'], res['roofline_step']['frac'],
                res['roofline_step_compulsory']['frac']))
        if world == 1 and not args.no_profile:
            # calibration: what torch's device-to-device copy reaches on THIS box (read + write bytes / time) -- a
            # reference point, not a ceiling (MI355X_MICROARCH.md quotes 6.29 TB/s for a float4 copy kernel); the
            # rooflines are quoted against the 8 TB/s specification
            ca = torch.empty(256 << 20, dtype=torch.float32, device=dev)          # 1 GiB
            cb = torch.empty_like(ca)
            for _ in range(2):
                cb.copy_(ca)
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record()
            for _ in range(10):
                cb.copy_(ca)
            c1.record()
            torch.cuda.synchronize()
            res['hbm_copy_GBps'] = 2 * ca.numel() * 4 * 10 / (c0.elapsed_time(c1) * 1e-3) / 1e9
            del ca, cb
            # the stand-alone multi-support SpMM of the same batch (gml_spmm_fwd: H = [A_s^T X]_s materialised), the
            # bandwidth-bound piece BASELINE.json's metric names: algorithmic bytes / mean launch time (HIP events)
            csr = data.csr('edge_index2')
            S_, Fin_ = int(data.edge_attr2.size(1)), 32
            xs = torch.randn(csr.N, Fin_, device=dev)
            vals = csr.sort_values(data.edge_attr2)
            for _ in range(3):
                Fn.spmm(csr, vals, xs, S_, Fin_)
            nrep, tblk = 20, []
            for _ in range(7):                                   # 7 blocks of 20 launches, median block
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(nrep):
                    Fn.spmm(csr, vals, xs, S_, Fin_)
                e1.record()
                torch.cuda.synchronize()
                tblk.append(e0.elapsed_time(e1) / nrep * 1e-3)
            t_s = float(np.median(tblk))
            q_s = 4 * (csr.E * S_ + csr.N * Fin_ + csr.N * S_ * Fin_) + 4 * (csr.E + csr.N + 1)
            res['spmm'] = {'kernel': 'gml_k_spectconv_fwd2<S, 0> via gml_spmm_fwd_ex (8-wave SpMM, H written; groups beyond its staging: gml_k_spmm3)', 'bound': 'hbm',
                           'achieved': q_s / t_s / 1e9, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': q_s / t_s / 1e9 / HBM_PEAK_GBS,
                           'avg_launch_ms': t_s * 1e3, 'algorithmic_bytes_per_launch': q_s, 'S': S_, 'Fin': Fin_,
                           'frac_of_copy_rate': q_s / t_s / 1e9 / res['hbm_copy_GBps'],
                           'blocks': len(tblk), 'launches_per_block': nrep, 'block_ms': [round(t * 1e3, 4) for t in tblk]}
            log('spmm (S = %d, Fin = %d, %d nodes): %.3f ms/launch = %.0f GB/s = %.3f of the HBM roof' % (
                S_, Fin_, csr.N, t_s * 1e3, q_s / t_s / 1e9, q_s / t_s / 1e9 / HBM_PEAK_GBS))
            del xs, vals
        if world == 1 and not args.no_profile and not args.no_extras:
            # ---- the same step with exact fp32 products (f32-input MFMA; bit-identical to an fmaf chain)
            Fn.F32_MFMA = True
            for _ in range(2):
                step()
            dtx, _ = timed_block(step, args.steps)
            Fn.PROFILE = {}
            timed_block(step, args.steps)                      # (a second, profiled block: HIP events per launch)
            profx, Fn.PROFILE = Fn.PROFILE, None
            candx, kmsx = rooflines(profx)
            Fn.F32_MFMA = False
            res['value_exact_fp32'] = dict(value=data.num_graphs * args.steps / dtx, unit='graphs/s', ms_per_step=dtx / args.steps * 1e3,
                                           arithmetic='exact fp32 (GML_F32_MFMA=1): f32-input MFMA conv kernels, the edge branch on the one-edge-per-lane fp32 family with the library tanh (round 5: before, it stayed on the bf16-split chains)',
                                           kernels_ms_per_step=kmsx)
            res['roofline_exact_fp32'] = candx[0]
            res['roofline_exact_fp32_other'] = candx[1:]
            log('exact fp32: %.3f ms/step' % (dtx / args.steps * 1e3))
            # ---- the same step with bf16 hi/lo pieces in the forward too (rounds 1-5's headline arithmetic)
            keep_ = Fn.EDGE_FWD6, Fn.FWD_F16
            Fn.EDGE_FWD6 = Fn.FWD_F16 = False
            for _ in range(2):
                step()
            dt3, _ = timed_block(step, args.steps)
            Fn.EDGE_FWD6, Fn.FWD_F16 = keep_
            res['value_bf16x3'] = dict(value=data.num_graphs * args.steps / dt3, unit='graphs/s', ms_per_step=dt3 / args.steps * 1e3,
                                       arithmetic='bf16 hi/lo pieces (three products per fp32 product) in every kernel, short tanh in the edge chain: GML_EDGE_FWD6=0 GML_FWD_F16=0')
            log('bf16x3 everywhere: %.3f ms/step' % (dt3 / args.steps * 1e3))
            # ---- the default arithmetic with EVERY support row evaluated (no sharing between an edge and its mirror)
            keep_s = Fn.EDGE_SYM
            Fn.EDGE_SYM = False
            for _ in range(2):
                step()
            dts, _ = timed_block(step, args.steps)
            Fn.EDGE_SYM = keep_s
            res['value_all_rows'] = dict(value=data.num_graphs * args.steps / dts, unit='graphs/s', ms_per_step=dts / args.steps * 1e3,
                                         note='GML_EDGE_SYM=0: the edge branch evaluates every support row, mirrors included')
            log('every support row evaluated: %.3f ms/step' % (dts / args.steps * 1e3))
            # ---- a NEW batch every step: the per-batch index work inside the timed region
            fields = {k: v for k, v in data.__dict__.items() if not k.startswith('_')}

            def fresh_step():
                return step(Batch(**fields))               # new Batch: CSR, group records, pre-split, source order rebuilt
            for _ in range(2):
                fresh_step()
            nfr = max(5, args.steps // 2)
            dtf, _ = timed_block(fresh_step, nfr)
            res['fresh_batch'] = dict(value=data.num_graphs * nfr / dtf, unit='graphs/s', ms_per_step=dtf / nfr * 1e3, steps=nfr,
                                      index_build_ms_per_batch=dtf / nfr * 1e3 - ms,
                                      note='every step builds CSR (both views), group records, the bf16 pre-split and the '
                                           'source-order copy of the supports for its batch inside the timed region')
            log('fresh batch: %.3f ms/step' % (dtf / nfr * 1e3))
        if world == 1 and not args.no_profile and not args.no_extras and args.distinct > 0:
            # ---- the same step over DISTINCT graphs (the headline batch tiles a pool of --pool graphs: bytes are honest, every
            #      128-row group pattern repeats 64 times; here degree ranks, window widths and LDS-cap fallbacks are sampled
            #      from every graph).  Supports by the device SpectralDesign.
            t_b = time.perf_counter()
            try:
                dd = build_batch_distinct(args.distinct, seed=31337, device=dev)
            except Exception as e:                             # noqa: BLE001
                dd = None
                res['distinct_graphs'] = dict(error=repr(e))
            if dd is not None:
                dd.csr('edge_index2')
                torch.cuda.synchronize()
                t_b = time.perf_counter() - t_b
                for _ in range(3):
                    step(dd)
                dtd, _ = timed_block(lambda: step(dd), args.steps)
                res['distinct_graphs'] = dict(value=dd.num_graphs * args.steps / dtd, unit='graphs/s', ms_per_step=dtd / args.steps * 1e3,
                                              graphs=dd.num_graphs, nodes=int(dd.x.size(0)), support_edges=int(dd.edge_index2.size(1)),
                                              build_seconds=t_b,
                                              note='%d distinct synthetic ZINC-like graphs (no tiling), supports built on the device '
                                                   '(gml_spectral_design); same model, step and timing as `value`' % dd.num_graphs)
                log('distinct graphs: %.3f ms/step (%d graphs, built in %.1f s)' % (dtd / args.steps * 1e3, dd.num_graphs, t_b))
                del dd
                torch.cuda.empty_cache()
        if world == 1 and not args.no_profile and not args.no_extras:
            # ---- the other BASELINE configs (parity-test cases, not bench lines): short runs with a roofline record each
            sys.path.insert(0, os.path.join(ROOT, 'tools'))
            try:                                               # (side measurements must never cost the headline line)
                import bench_configs
                res['other_configs'] = bench_configs.run(dev, quick=False)
                for oc in res['other_configs']:
                    log('other config %s: %.3f ms/step, %.2f M graphs/s' % (oc['config'], oc['ms_per_step'], oc['graphs_per_s'] / 1e6))
            except Exception as e:                             # noqa: BLE001
                res['other_configs'] = dict(error=repr(e))
            # ---- config 5 as SURVEY s8(d) specifies it: the 15 real sr25 graphs tiled to >= 1 M nodes, S in {6, 12, 24, 48}:
            #      stand-alone SpMM GB/s against the roof per S + the forward-only model (sr25.py:282-300)
            try:
                import bench_sr25_sweep
                res['sr25_sweep'] = bench_sr25_sweep.run(dev)
                for r5 in res['sr25_sweep']:
                    log('sr25 sweep S=%d: SpMM %.2f of the HBM roof (Fin 32), %.2f (Fin 48); forward %.2f ms' % (
                        r5['S'], r5['spmm_Fin32']['frac'], r5['spmm_Fin48']['frac'], r5['forward']['ms']))
            except Exception as e:                             # noqa: BLE001
                res['sr25_sweep'] = dict(error=repr(e))
            # ---- config 4 (MNIST-75, the config BASELINE.json shards over 8 GPUs): dense-block train step at 1,024 graphs per GPU
            try:
                import subprocess as _sp
                r4 = _sp.run([sys.executable, os.path.join(ROOT, 'tools', 'bench_mnist.py'), '1024', 'dense'], capture_output=True, text=True, timeout=300)
                res['mnist75'] = json.loads(r4.stdout.strip().splitlines()[-1])
                log('mnist75 dense-block step: %.3f ms, %.0f k graphs/s' % (res['mnist75']['dense']['ms_per_step'], res['mnist75']['dense']['graphs_per_s'] / 1e3))
            except Exception as e:                             # noqa: BLE001
                res['mnist75'] = dict(error=repr(e))
        if world == 1 and args.ref_batch > 0:
            # the reference's own batch size: launch-latency bound, so the step is replayed from a HIP graph
            rb, _ = build_batch(args.ref_batch, args.ref_batch, seed=7, device=dev)
            rb.csr('edge_index2')
            torch.manual_seed(0)
            rm = models.zinc_gnnml3().to(dev)
            from gnn_matlang_amd.optim import OneLaunchAdam      # Adam as ONE launch (gml_adam_many), step count on the device
            o = OneLaunchAdam(rm.parameters(), lr=1e-3)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                      # warm-up on a side stream (allocator, lazy init)
                for _ in range(3):
                    o.zero_grad(set_to_none=True)
                    models.zinc_step_loss(rm, rb).backward()
                    o.step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                o.zero_grad(set_to_none=True)               # gradients are handed over, not accumulated
                gl = models.zinc_step_loss(rm, rb)
                with Fn.deferred_folds(list(rm.parameters())):
                    gl.backward()
                o.step()
            for _ in range(20):
                gr.replay()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            nrep = 200
            for _ in range(nrep):
                gr.replay()
            torch.cuda.synchronize()
            dt1 = (time.perf_counter() - t1) / nrep
            res['ref_batch'] = dict(graphs_per_step=rb.num_graphs, ms_per_step=dt1 * 1e3, value=rb.num_graphs / dt1,
                                    unit='graphs/s', mode='ONE batch, whole step replayed from one HIP graph (launch-latency '
                                    'floor of this batch size; see epoch_bs64 for distinct batches)',
                                    final_loss=float(gl.item()))
            log('reference batch %d: %.3f ms/step (HIP graph)' % (rb.num_graphs, dt1 * 1e3))
            if not args.no_extras:
                # ---- one epoch of Zinc12k.py:354-371 over 10,000 distinct synthetic graphs: shuffled, batch 64, every
                #      batch assembled on the device and indexed inside the loop (eager launches, no graph replay)
                from gnn_matlang_amd import SpectralDesign, synthetic
                from gnn_matlang_amd.dataset import DeviceDataset
                raw = synthetic.make_graphs('zinc', 10000, seed=4242)
                dsd = DeviceDataset.from_graphs(SpectralDesign(recfield=2, dv=2, nfreq=7).design_many(raw), dev)
                torch.manual_seed(0)
                em = models.zinc_gnnml3().to(dev)
                eo = torch.optim.Adam(em.parameters(), lr=1e-3, fused=True)
                gen = torch.Generator().manual_seed(1)

                def epoch():
                    tot = torch.zeros((), device=dev)
                    nb = 0
                    for b in dsd.epoch(args.ref_batch, generator=gen):
                        eo.zero_grad(set_to_none=True)
                        l = models.zinc_loss(em(b), b.y)
                        l.backward()
                        eo.step()
                        tot += l.detach()                      # (no .item() per step: the reference syncs at Zinc12k.py:369)
                        nb += 1
                    return tot, nb
                epoch()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                tot, nb = epoch()
                torch.cuda.synchronize()
                dt2 = time.perf_counter() - t2
                eager = dict(seconds=dt2, value=len(dsd) / dt2, ms_per_step=dt2 / nb * 1e3, mean_loss=float(tot.item()) / len(dsd),
                             mode='eager: per batch device-side assembly from the HBM-resident data set (one host read for the '
                                  'sizes), CSR + group records + pre-split built, fwd + loss + bwd + fused Adam')
                log('epoch at batch %d, eager: %.3f s for %d graphs (%.3f ms/step)' % (args.ref_batch, dt2, len(dsd), dt2 / nb * 1e3))
                # ---- eager again, over static-shape batches from gml_batch_assemble (no host read per batch, no HIP graph)
                dsd.y = dsd.y.float()
                bd_e = dsd.bounds(args.ref_batch)

                def epoch_static():
                    tot = torch.zeros((), device=dev)
                    nb = 0
                    Bq_ = args.ref_batch
                    for b in dsd.epoch_static(args.ref_batch, generator=gen, bounds=bd_e):
                        eo.zero_grad(set_to_none=True)
                        pre = em(b)
                        l = ((pre[:Bq_, 0] - b.y[:Bq_]).abs() * b.graph_valid).sum()
                        l.backward()
                        eo.step()
                        tot += l.detach()
                        nb += 1
                    return tot, nb
                epoch_static()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                tot_s, nb_s = epoch_static()
                torch.cuda.synchronize()
                dt2s = time.perf_counter() - t2
                eager['static_batches'] = dict(seconds=dt2s, value=len(dsd) / dt2s, ms_per_step=dt2s / nb_s * 1e3, mean_loss=float(tot_s.item()) / len(dsd),
                                               mode='eager over DeviceDataset.epoch_static: one gml_batch_assemble launch per batch, no host read, no HIP graph')
                log('epoch at batch %d, eager over static batches: %.3f ms/step' % (args.ref_batch, dt2s / nb_s * 1e3))
                # ---- the same epoch as ONE captured HIP graph replayed per batch: static padded shapes (bounds of the data
                #      set), batch assembly + index build + fwd + loss + bwd + Adam all inside the graph, no host read
                bd = dsd.bounds(args.ref_batch)
                G_, Bq = len(dsd), args.ref_batch
                ids_buf = torch.zeros(Bq, dtype=torch.int64, device=dev)
                dsd.prepare()                                  # once per data set: every graph's own index structure + pre-split supports

                def captured_epoch(assemble):
                    torch.manual_seed(0)
                    cm = models.zinc_gnnml3().to(dev)
                    from gnn_matlang_amd.optim import OneLaunchAdam      # Adam as ONE launch (gml_adam_many), step count on the device
                    co = OneLaunchAdam(cm.parameters(), lr=1e-3)
                    loss_acc = torch.zeros((), device=dev)
                    one_ = torch.ones((), device=dev)

                    def padded_step():
                        b = assemble(ids_buf, bd)
                        co.zero_grad(set_to_none=True)
                        l = models.zinc_step_loss(cm, b, loss_sum=loss_acc)                               # L1-sum over the real graphs (Zinc12k.py:365); head + loss: one launch each way
                        with Fn.deferred_folds(list(cm.parameters())):                 # the twelve partial-sum folds of the backward as ONE launch
                            l.backward(one_)                                           # (a resident unit gradient: no fill launch per step)
                        co.step()
                    ids_buf.copy_(torch.arange(Bq, device=dev))
                    side2 = torch.cuda.Stream()
                    side2.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side2):
                        for _ in range(3):
                            padded_step()
                    torch.cuda.current_stream().wait_stream(side2)
                    torch.cuda.synchronize()
                    cg = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(cg):
                        padded_step()
                    egen = torch.Generator().manual_seed(7)

                    def graph_epoch():
                        perm = torch.randperm(G_, generator=egen).to(dev)
                        perm = torch.cat([perm, torch.full(((-G_) % Bq,), G_, dtype=torch.int64, device=dev)])   # last batch: absent graphs
                        loss_acc.zero_()
                        for i in range(0, perm.numel(), Bq):
                            ids_buf.copy_(perm[i:i + Bq])
                            cg.replay()
                        return perm.numel() // Bq
                    graph_epoch()
                    torch.cuda.synchronize()
                    t3 = time.perf_counter()
                    nb3 = graph_epoch()
                    torch.cuda.synchronize()
                    return time.perf_counter() - t3, nb3, float(loss_acc.item())
                dt_t, _, loss_t = captured_epoch(dsd.batch_padded)          # round-3 road: torch gathers + the general CSR build per batch
                dt3, nb3, loss3 = captured_epoch(dsd.batch_assembled)       # one launch from the per-graph structure (gml_batch_assemble)
                log('epoch at batch %d, captured, torch assembly + CSR build per batch: %.3f ms/step (loss %.6f vs %.6f: %s)' % (
                    Bq, dt_t / nb3 * 1e3, loss_t / G_, loss3 / G_, 'identical' if loss_t == loss3 else 'DIFFERENT'))
                res['epoch_bs64'] = dict(graphs=G_, batches=nb3, batch_size=Bq, seconds=dt3, value=G_ / dt3, unit='graphs/s',
                                         ms_per_step=dt3 / nb3 * 1e3, mean_loss=loss3 / G_,
                                         mode='one HIP graph replayed per batch: static padded shapes (%d nodes, %d support edges '
                                              'for <= %d graphs), batch + both CSR views + pre-split supports in ONE launch from the '
                                              'per-graph structure computed once per data set (gml_batch_assemble) + group records + '
                                              'fwd + L1-sum loss + bwd + fused Adam inside the graph, distinct shuffled batches, '
                                              'no host read' % (bd['n_pad'], bd['e2_pad'], Bq),
                                         torch_assembly=dict(ms_per_step=dt_t / nb3 * 1e3, mean_loss=loss_t / G_, same_loss=loss_t == loss3,
                                                             mode='round-3 road: torch gathers + general CSR build inside the graph'),
                                         eager=eager)
                log('epoch at batch %d, captured: %.3f s for %d graphs (%.3f ms/step)' % (Bq, dt3, G_, dt3 / nb3 * 1e3))
        if world == 1 and not args.no_cpu:
            res['cpu_baseline'] = cpu_baseline(args.cpu_graphs, log)
            if base is not None and data.num_graphs % base.num_graphs == 0:
                # ---- checker leg (the oracle as the CHECKER, never the thing measured): the headline batch, one step per arithmetic
                # mode, logits and every parameter gradient against the oracle in float64 under the term-sum criterion
                # (oracle/parity_at_size.py; the same check as tests/test_gpu_parity.py::test_bench_size_train_step_vs_fp64_oracle)
                # Two states.  The INITIAL parameters are the pinned one (the figures are reproducible and held to 1e-4 by the GPU test).
                # The parameters the timed steps leave are reported as they come: after hundreds of Adam steps on random targets some units
                # are nearly dead; the headline mode's forward error (1e-5 of a layer's scale) then shows as relu units on the other side
                # of zero (counted per layer) and as large relative errors of small activations -- elements of nearly dead units' gradients
                # exceed 1e-4 of their own term sums (DESIGN s6); the exact mode and the CPU fp32 reference stay at 1e-6.
                res['parity_vs_oracle_after_training'] = parity_vs_oracle(model, data, base, log)
                res['parity_vs_oracle_after_training']['state'] = 'parameters after the timed steps of this run (informational: see relu_units_on_the_other_side_of_zero)'
                if parity0 is not None:
                    res['parity_vs_oracle'] = parity0
                # per mode: worst element of any parameter gradient relative to its layer-local term sum (inputs of the layer taken as
                # exact: the strict form), at the parameters this run ended with; logits relative to max |logit|
                pick = lambda rec: {k: dict(gradients_termsum=v['max_rel_err_termsum'], logits=v['logits_rel_err'])
                                    for k, v in rec['modes'].items() if 'max_rel_err_termsum' in v}
                if parity0 is not None:
                    res['max_rel_err_vs_oracle'] = pick(parity0)                       # (initial parameters: the pinned state)
                res['max_rel_err_vs_oracle_after_training'] = pick(res['parity_vs_oracle_after_training'])
        if args.full:
            where = write_extras(res)
            res['extras'] = 'bench_extras.json'
            log('full record (%d characters): %s' % (len(json.dumps(res)), ', '.join(where) or 'not written'))
        sys.stdout.flush()
        print(compact_line(res), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
