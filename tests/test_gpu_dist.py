"""Two ranks on the GPU with the PRODUCT model: the data-parallel step through libgml_hip.so (FlatGradSync handing
p.grad views of the flat buffer to the fused Adam) reproduces the reference's full-batch gradients and loss trajectory.
The ranks are fresh child processes started under torch.distributed.run (never a re-exec of this process); both use
cuda:0 with the gloo backend -- RCCL needs one device per rank, which the 1-GPU test box does not have (the 8-GPU
bench runs the same code path with backend 'nccl')."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, rel_err

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize('balanced', [0, 1])
def test_two_ranks_product_model_equals_reference_full_batch(tmp_path, balanced):
    out = str(tmp_path / 'r0.pt')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(ROOT, 'tests', '_dist_gpu_worker.py'), out, str(balanced)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='1'))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = torch.load(out)
    assert res['world'] == 2
    g = np.load(os.path.join(GOLDEN, 'model_zinc_gnnml3.npz'))
    for n, v in res['grads'].items():                    # == the reference's full-batch gradients (1e-4 of the tensor's scale)
        ref = g['grad/' + n]
        assert np.abs(v.numpy() - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-30), n
    np.testing.assert_allclose(res['losses'], g['loss_traj'][:3], rtol=1e-4)


def _run_bench(extra, timeout=900):
    import json
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', '--no-cpu', '--no-extras',
           '--ref-batch', '0', '--min-seconds', '0'] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0'))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_strong_scaling_shards_one_global_batch():
    """--global-batch: ONE global data set cut by graph.shard_graphs_balanced (sum of support edges); with one rank the cut is
    the whole set -- checks the sharding code path and its record on the 1-GPU box."""
    d = _run_bench(['--gpus', '1', '--global-batch', '4096'])
    assert d['scaling'] == 'strong' and d['config']['global_batch'] == 4096
    sh = d['sharding']
    assert sh['graphs_per_rank'] == [4096] and sh['support_edges_per_rank'][0] == d['config']['support_edges_per_gpu']
    assert abs(sh['max_over_mean'] - 1.0) < 1e-12


def test_bench_dump_outputs_after_exactly_the_requested_steps(tmp_path):
    """--dump-outputs writes the last timed step's loss, parameters and gradients.  --steps is the exact number of timed steps:
    1 warm-up + 3 timed and 2 warm-up + 2 timed are the same four steps on the same seeded inputs, in two fresh processes, so
    every array agrees (one more Adam step would move the parameters by ~1e-3) -- also when the first run settles the GPU for
    --min-seconds on a copy of the model before its timed steps."""
    runs = []
    for warm, steps, settle in ((1, 3, '0.5'), (2, 2, '0')):
        out = tmp_path / ('w%d_s%d' % (warm, steps))
        d = _run_bench(['--gpus', '1', '--batch', '2048', '--no-profile', '--warmup', str(warm), '--steps', str(steps),
                        '--min-seconds', settle, '--dump-outputs', str(out)])
        assert d['steps'] == steps
        runs.append({f[:-4]: np.load(out / f) for f in os.listdir(out)})
    a, b = runs
    assert set(a) == set(b) and 'loss' in a and len(a) == 1 + 2 * len([k for k in a if k.startswith('param.')])
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        assert rel_err(a[k], b[k]) <= 1e-5, (k, rel_err(a[k], b[k]))


def test_bench_plain_run_takes_no_side_measurements(tmp_path):
    """A plain run prints the headline alone and writes no full record; --full takes the side measurements (here the per-kernel
    profile and its rooflines) after the same timed steps, whose outputs agree with the plain run's."""
    runs = []
    for extra in ([], ['--full']):
        out = tmp_path / ('full' if extra else 'plain')
        d = _run_bench(['--gpus', '1', '--batch', '2048', '--dump-outputs', str(out)] + extra)
        assert d['steps'] == 3 and d['warmup'] == 1 and d['ms_per_step'] > 0 and np.isfinite(d['value'])
        runs.append((d, {f[:-4]: np.load(out / f) for f in os.listdir(out)}))
    (plain, a), (full, b) = runs
    for k in ('roofline', 'kernels_ms_per_step', 'edge_unique_rows', 'extras'):
        assert k not in plain and k in full, k
    assert set(a) == set(b)
    for k in a:
        assert rel_err(a[k], b[k]) <= 1e-5, (k, rel_err(a[k], b[k]))


def test_bench_two_ranks_share_the_device_over_gloo():
    """bench.py's N > 1 code path on the 1-GPU box: two spawned ranks on cuda:0 over gloo
    (GML_BENCH_SHARE_DEVICE=1) -- sharded batch, flat all-reduce per step, per-rank times, all-reduce timing and the captured
    batch-64 step (gloo collectives cannot be captured: that record carries the error string here, the graph on RCCL)."""
    import json
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '2', '--warmup', '1', '--full', '--no-cpu', '--no-extras', '--ref-batch', '0',
           '--min-seconds', '0', '--gpus', '2', '--batch', '2048']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', GML_BENCH_SHARE_DEVICE='1'))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d['n_gpus'] == 2 and d['n_ranks_seen'] == 2 and d['config']['global_batch'] == 4096
    dp = d['data_parallel']
    assert len(dp['per_rank_ms_per_step']) == 2 and dp['allreduce_ms'] > 0 and dp['allreduce_bytes'] == 4 * d['config']['params']
    assert 'captured_bs64_per_rank' in dp


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs: RCCL wants one device per rank')
def test_bench_two_gpus_over_rccl():
    """the real entry point on the first box that has two GPUs: bench.py --gpus 2 spawns its ranks, backend nccl (= RCCL),
    one flat SUM all-reduce per step; weak scaling and the edge-balanced strong-scaling cut"""
    d = _run_bench(['--gpus', '2', '--batch', '4096'])
    assert d['n_gpus'] == 2 and d['n_ranks_seen'] == 2 and d['rccl_version']
    assert d['config']['global_batch'] == 8192 and np.isfinite(d['final_loss'])
    d = _run_bench(['--gpus', '2', '--global-batch', '8192'])
    assert d['n_ranks_seen'] == 2 and d['scaling'] == 'strong' and sum(d['sharding']['graphs_per_rank']) == 8192
    assert d['sharding']['max_over_mean'] < 1.02


def test_bench_strong_scaling_four_ranks_share_the_device():
    """--global-batch (strong scaling) with FOUR spawned ranks on cuda:0 over gloo (GML_BENCH_SHARE_DEVICE=1): ONE
    global data set cut by shard_graphs_balanced into four shards balanced by support edges, one flat all-reduce per step, per-rank
    times -- and the captured batch-64 step records an error string instead of hanging where the collective cannot be captured (gloo)."""
    import json
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '2', '--warmup', '1', '--full', '--no-cpu', '--no-extras', '--ref-batch', '0',
           '--min-seconds', '0', '--gpus', '4', '--global-batch', '4096']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', GML_BENCH_SHARE_DEVICE='1'))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = r.stdout.strip().splitlines()[-1]
    assert len(line) < 8000
    d = json.loads(line)
    assert d['n_gpus'] == 4 and d['n_ranks_seen'] == 4 and d['scaling'] == 'strong' and d['config']['global_batch'] == 4096
    sh = d['sharding']
    assert len(sh['graphs_per_rank']) == 4 and sum(sh['graphs_per_rank']) == 4096 and sh['max_over_mean'] < 1.05
    dp = d['data_parallel']
    assert len(dp['per_rank_ms_per_step']) == 4 and dp['allreduce_ms'] > 0 and dp['allreduce_bytes'] == 4 * d['config']['params']
    cap = dp['captured_bs64_per_rank']
    assert ('error' in cap) or (cap.get('ms_per_step', 0) > 0), cap          # gloo: an error string; RCCL: the captured step's time
    assert np.isfinite(d['final_loss'])
