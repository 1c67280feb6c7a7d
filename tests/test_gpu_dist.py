"""Sample-sharded sampling with the real engine on more than one process: 2 ranks on the one visible GPU, gloo
rendezvous, fresh child processes.  `sample_and_decode_sharded` keys class ids and Philox noise by the GLOBAL sample index
(`sample_offset`), so the gathered result of the ragged 3 + 2 split must equal the unsharded run of the same global batch bit
for bit -- codes AND pixels (EXACT arithmetic is batch-invariant)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_ranks(tmp_path, world, gb, steps, mode):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / f'sharded_{mode}.npz')
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', 'dist_gpu_worker.py'), out, str(gb), str(steps), mode],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    return np.load(out), json.load(open(out + '.json'))


@pytest.mark.parametrize('mode', ['exact', 'fast'])
def test_two_ranks_on_one_gpu_equal_the_unsharded_run(tmp_path, mode):
    gb, steps = 5, 64
    got, info = run_ranks(tmp_path, 2, gb, steps, mode)
    sys.path.insert(0, ROOT)
    from hqtransformer_amd import synth
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.sampling import sampling_ihqgpt
    dev = torch.device('cuda:0')
    model = ImageGPT2(load_config(os.path.join(ROOT, 'configs', 'tiny-cls.yaml')), seed=5).to(dev)
    cond = torch.from_numpy(synth.class_ids(7, gb, model.stage2.spec.n_classes))
    fast = mode == 'fast'
    # FAST draws are reproducible per (seed, schedule): the ranks of this test share one GPU and therefore run the launch chain (HQT_PERSIST=0 in
    # dist_gpu_worker.py) -- the unsharded run they are compared with bit for bit must take the same schedule, not the persistent chain
    os.environ['HQT_PERSIST'] = '0'
    try:
        ct, cb = sampling_ihqgpt(model.stage2, num_candidates=gb, cond=cond, top_k_top=50, top_p_top=0.9, top_k_bot=None, top_p_bot=None,
                                 softmax_temperature=[1.0, 0.9], use_fp16=fast, is_tqdm=False, max_seq_len=steps, seed=1234, sample_offset=0)
        px = model.stage1.decode_sequences(ct, cb, precision='fast' if fast else 'exact')
        torch.cuda.synchronize()
    finally:
        del os.environ['HQT_PERSIST']
    assert np.array_equal(got['codes_top'], ct.cpu().numpy()) and np.array_equal(got['codes_bot'], cb.cpu().numpy())
    if fast:       # bf16 GEMM tiles depend on the row count (3 / 2 / 5 rows pad differently): same codes, pixels to bf16 accuracy
        assert np.abs(got['pixels'] - px.cpu().numpy()).max() <= 0.05
    else:
        assert np.array_equal(got['pixels'], px.cpu().numpy())
    assert len(info['host_ms_per_submit_3_lanes']) == 2
    print('host ms per submitted step (3 lanes) per rank:', [round(v, 3) for v in info['host_ms_per_submit_3_lanes']])


def test_eight_ranks_ragged_global_batch_equal_the_unsharded_run(tmp_path):
    """The 8-rank shape of BASELINE configs[2] on one GPU: a global batch of 13 samples over 8 processes (slices 2 2 2 2 2 1 1 1), every
    rank its own engine on the shared device, one gather to rank 0 -- codes and pixels equal the unsharded run bit for bit (EXACT)."""
    gb, steps = 13, 64
    got, info = run_ranks(tmp_path, 8, gb, steps, 'exact')
    sys.path.insert(0, ROOT)
    from hqtransformer_amd import synth
    from hqtransformer_amd.config import load_config
    from hqtransformer_amd.models import ImageGPT2
    from hqtransformer_amd.sampling import sampling_ihqgpt
    dev = torch.device('cuda:0')
    model = ImageGPT2(load_config(os.path.join(ROOT, 'configs', 'tiny-cls.yaml')), seed=5).to(dev)
    cond = torch.from_numpy(synth.class_ids(7, gb, model.stage2.spec.n_classes))
    ct, cb = sampling_ihqgpt(model.stage2, num_candidates=gb, cond=cond, top_k_top=50, top_p_top=0.9, top_k_bot=None, top_p_bot=None,
                             softmax_temperature=[1.0, 0.9], use_fp16=False, is_tqdm=False, max_seq_len=steps, seed=1234, sample_offset=0)
    px = model.stage1.decode_sequences(ct, cb, precision='exact')
    torch.cuda.synchronize()
    assert got['codes_top'].shape[0] == gb
    assert np.array_equal(got['codes_top'], ct.cpu().numpy()) and np.array_equal(got['codes_bot'], cb.cpu().numpy())
    assert np.array_equal(got['pixels'], px.cpu().numpy())
    assert len(info['host_ms_per_submit_3_lanes']) == 8


def _bench_two_ranks(extra_env, gpus_needed, world=2):
    if torch.cuda.device_count() < gpus_needed:
        pytest.skip(f'needs {gpus_needed} visible GPUs (this box has {torch.cuda.device_count()})')
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(ROOT, 'bench.py'), '--gpus', str(world), '--steps', '6', '--warmup', '2', '--merge', '2', '--inflight', '2',
           '--config', os.path.join(ROOT, 'configs', 'tiny-cls.yaml'), '--full', '--no-cpu-baseline', '--no-roofline']
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', **extra_env), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith('{')][-1]
    return json.loads(line)


def test_bench_two_ranks_control_flow_on_one_gpu():
    """`bench.py --gpus 2` exactly as the driver launches it (torch.distributed.run, one process per rank), on boxes with a single GPU:
    HQT_BENCH_SHARE_GPU=1 maps both ranks onto the visible device and rendezvous runs over gloo -- the N > 1 control flow (default
    `--gather pixels`, its pre-flight, barrier + max-over-ranks timing, per-rank host times, one JSON line from rank 0); the numbers
    mean nothing."""
    d = _bench_two_ranks({'HQT_BENCH_SHARE_GPU': '1'}, 1)
    assert d['n_gpus'] == 2 and d['config']['global_batch'] == 2 * d['config']['per_gpu_batch'] and d['scaling'] == 'weak'
    # gloo cannot gather device tensors: the pre-flight then drops the gather and says so -- the fallback the RCCL run relies on
    assert d['config']['gather'].startswith(('pixels', 'none (requested gather failed')), d['config']['gather']
    assert len(d['host_ms_per_step_ranks']) == 2 and d['value'] > 0


def test_bench_eight_ranks_control_flow_on_one_gpu():
    """The driver's 8-GPU launch (`torch.distributed.run --nproc-per-node 8 bench.py --gpus 8`) rehearsed on ONE GPU: eight processes share
    the visible device (HQT_BENCH_SHARE_GPU=1, gloo rendezvous).  What runs: rank / world bookkeeping, the gather pre-flight and its
    fall-back (gloo cannot gather device tensors), rank 0's receive buffers for 8 ranks, the barrier + max-over-ranks timing, eight per-rank
    host costs (the box grants 16 cores to the 8 processes), ONE JSON line from rank 0 with n_gpus = 8 and a weak-scaling global batch.
    The numbers mean nothing: eight engines time-share one GPU."""
    d = _bench_two_ranks({'HQT_BENCH_SHARE_GPU': '1'}, 1, world=8)
    assert d['n_gpus'] == 8 and d['config']['global_batch'] == 8 * d['config']['per_gpu_batch'] and d['scaling'] == 'weak'
    assert d['config']['gather'].startswith(('pixels', 'none (requested gather failed')), d['config']['gather']
    assert len(d['host_ms_per_step_ranks']) == 8 and all(v > 0 for v in d['host_ms_per_step_ranks']) and d['value'] > 0
    # skew visibility: every rank's own wall time and images/s travel with the max-over-ranks line
    assert len(d['elapsed_s_ranks']) == 8 and len(d['value_ranks']) == 8 and all(v > 0 for v in d['value_ranks'])
    assert abs(d['value'] - 8 * d['config']['per_gpu_batch'] * d['steps'] / max(d['elapsed_s_ranks'])) <= 0.02 * d['value']
    print('8 ranks on one GPU: host ms per step per rank', d['host_ms_per_step_ranks'], 'unthrottled', d.get('host_ms_per_step_unthrottled'))


def test_bench_two_gpus_over_rccl():
    """The same launch on two real GPUs: the nccl (= RCCL) backend, `dist.gather` of every step's pixels to rank 0 inside the timed
    region (BASELINE configs[2]).  Skipped on one-GPU boxes -- the round-end multi-GPU run of the driver is then the first time this
    branch executes; the gather is pre-flighted there and the line says so if it had to be dropped."""
    d = _bench_two_ranks({}, 2)
    assert d['n_gpus'] == 2 and d['config']['gather'].startswith('pixels'), d['config']['gather']


def _bench_direct(args, extra_env):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py')] + args + ['--steps', '6', '--warmup', '2', '--merge', '2', '--inflight', '2',
           '--config', os.path.join(ROOT, 'configs', 'tiny-cls.yaml'), '--full', '--no-cpu-baseline', '--no-roofline', '--no-exact-mode']
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT')}
    r = subprocess.run(cmd, cwd=ROOT, env=dict(env, HSA_ENABLE_IPC_MODE_LEGACY='0', **extra_env), capture_output=True, text=True, timeout=900)
    return r


def test_bench_gpus_flag_without_a_launcher_starts_its_own_ranks():
    """`python bench.py --gpus 2` with WORLD_SIZE unset (how the driver called `--gpus 1` in round 3): bench.py must start the two ranks
    itself (a child torch.distributed.run) and print a 2-GPU line -- never a 1-GPU number under a 2-GPU flag.  Two ranks share the one
    visible GPU through the HQT_BENCH_SHARE_GPU hook; without the hook the same command must refuse (fewer devices than ranks)."""
    r = _bench_direct(['--gpus', '2'], {'HQT_BENCH_SHARE_GPU': '1'})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert d['n_gpus'] == 2 and d['config']['global_batch'] == 2 * d['config']['per_gpu_batch']
    assert d['gather_ok'] in (True, False) and 'like_for_like' in d
    if torch.cuda.device_count() < 2:
        r = _bench_direct(['--gpus', '2'], {})
        assert r.returncode != 0 and 'refusing' in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith('{')]


def test_bench_rccl_branch_with_one_rank():
    """The nccl (= RCCL) branch of bench.py on a one-GPU box: HQT_BENCH_FORCE_DIST=1 makes the plain 1-GPU run create a ONE-rank RCCL
    process group, so init_process_group('nccl'), the gather pre-flight, `dist.gather` of every step's pixels on the lane's stream,
    the barrier and the max-over-ranks all execute on RCCL (with two GPUs test_bench_two_gpus_over_rccl runs the real thing)."""
    r = _bench_direct(['--gpus', '1'], {'HQT_BENCH_FORCE_DIST': '1'})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert d['n_gpus'] == 1 and d['config']['gather'].startswith('pixels'), d['config']['gather']
    assert d['gather_ok'] is True
