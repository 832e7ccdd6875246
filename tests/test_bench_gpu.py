"""bench.py's N > 1 path end to end on one GPU: `bench.py --gpus 2` starts
its two ranks itself (no torchrun), both on device 0 over the gloo staged
transport (the rehearsal knobs; RCCL refuses two ranks on one device), runs
the recursive-halving reduce-scatter value leg with its bit-exact parity gate,
and rank 0's one line carries n_gpus = 2, the schedule that ran and the
defaults A/B; then the same under torch.distributed.run, the driver's own N > 1
form."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_gpus_2_self_launched_line():
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env.update(MPIX_BENCH_SAME_DEVICE='1', MPIX_BENCH_BACKEND='gloo')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2',
                        '--steps', '2', '--warmup', '1', '--count', str(1 << 22),
                        '--rsb-bytes', str(16 << 20), '--full', '--no-extras'],
                       cwd=ROOT, capture_output=True, text=True, timeout=100, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['schedule_ran'] == 'recursive_halving', d
    assert d['parity']['bit_exact_all_ranks'] and d['value'] > 0, d
    # the timed result itself, at the timed size, on every rank
    assert d['parity']['full_size_bit_exact_all_ranks'], d['parity']
    assert d['parity']['full_size_recvcount'] == (16 << 20) // 4 // 2, d['parity']
    # the overlap x store-policy defaults
    # timed beside the shipped one, every variant first bit-exact on every
    # rank against the association (not against the default's own output)
    ab = d['defaults_ab']
    for k in ('overlap_on_policy_on', 'overlap_off_policy_on', 'overlap_on_policy_off',
              'overlap_off_policy_off'):
        assert ab[k]['bit_exact_vs_association_all_ranks'] and ab[k]['ms_per_step'] > 0, ab
    # the reference schedule's host work as the baseline
    c = d['cpu_baseline']
    assert c['kind'] == 'port' and c['cores'] == 2 and c['value'] > 0, c


@pytest.mark.gpu
def test_bench_full_size_check_catches_a_flipped_bit():
    """the full-size check is live: one bit flipped in rank 1's timed result
    (MPIX_BENCH_FAULT_RANK, a test hook) fails the run with EXIT_PARITY and a
    top-level error naming the timed size"""
    sys.path.insert(0, ROOT)
    import bench
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env.update(MPIX_BENCH_SAME_DEVICE='1', MPIX_BENCH_BACKEND='gloo', MPIX_BENCH_FAULT_RANK='1')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2',
                        '--steps', '2', '--warmup', '1', '--count', str(1 << 22),
                        '--rsb-bytes', str(16 << 20), '--full', '--no-extras', '--no-cpu-baseline',
                        '--no-ab'], cwd=ROOT, capture_output=True, text=True, timeout=100, env=env)
    assert p.returncode == bench.EXIT_PARITY, (p.returncode, p.stderr[-3000:])
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][0])
    assert d['value'] is None and 'timed size' in d['error'], d


@pytest.mark.gpu
def test_bench_gpus_2_under_torchrun_line():
    """the same line in the driver's own N > 1 form, `python -m
    torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1
    --master-port P bench.py --gpus 2 ...`: the ranks run as the launcher gives
    them (WORLD_SIZE set, no self-launch) and rank 0's one line is the N-rank
    line"""
    sys.path.insert(0, ROOT)
    import bench
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR')}
    env.update(MPIX_BENCH_SAME_DEVICE='1', MPIX_BENCH_BACKEND='gloo')
    p = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
                        '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                        '--master-port', str(bench.free_port()), os.path.join(ROOT, 'bench.py'),
                        '--gpus', '2', '--steps', '2', '--warmup', '1', '--count', str(1 << 22),
                        '--rsb-bytes', str(16 << 20), '--full', '--no-extras', '--no-cpu-baseline'],
                       cwd=ROOT, capture_output=True, text=True, timeout=110, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['launcher'] == 'external', d
    assert d['schedule_ran'] == 'recursive_halving' and d['parity']['bit_exact_all_ranks'], d
    for k in ('overlap_on_policy_on', 'overlap_off_policy_on', 'overlap_on_policy_off',
              'overlap_off_policy_off'):
        assert d['defaults_ab'][k]['bit_exact_vs_association_all_ranks'], d['defaults_ab']
    assert d['parity']['full_size_bit_exact_all_ranks'], d['parity']


HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def _bench_n1(extra, count):
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
                        '--steps', '3', '--warmup', '2', '--count', str(count)] + extra,
                       cwd=ROOT, capture_output=True, text=True, timeout=100, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize('count', [(1 << 20) + 3, (1 << 23) + 5])
def test_plain_run_is_the_headline_alone_and_dumps_its_result(tmp_path, count):
    """a plain `--gpus 1 --steps N --warmup W` run prints the headline and
    none of the --full figures, and --dump-outputs writes inout as the last
    timed step left it: the seeded operands folded 1 + W + N times (one IEEE
    fp32 add per element and call, so the bits are fixed) -- whole at the
    small count, the seeded sample of it past the size limit"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    d = _bench_n1(['--dump-outputs', str(tmp_path / 'out')], count)
    for k in HEADLINE:
        assert d[k] is not None, (k, d)
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 2 and d['unit'] == 'GiB/s'
    assert d['higher_is_better'] is True and d['dtype'] == 'f32' and d['metric'] == bench.METRIC
    assert d['ms_per_step'] > 0 and d['config']['count'] == count
    assert abs(d['value'] - 3 * count * 4 / (d['ms_per_step'] * 1e-3) / bench.GIB) <= 0.01 * d['value']
    for k in ('roofline', 'cpu_baseline', 'host_crossover', 'sync_call_latency', 'configs_3_and_5'):
        assert k not in d, k
    assert os.listdir(tmp_path / 'out') == ['reduce_local_inout.npy']
    got = np.load(tmp_path / 'out' / 'reduce_local_inout.npy')
    dev = torch.device('cuda', 0)
    inout = torch.empty(count, dtype=torch.float32, device=dev)
    inb = torch.empty(count, dtype=torch.float32, device=dev)
    bench.fill_uniform(inout, 0x5EED0001)
    bench.fill_uniform(inb, 0x5EED0002)
    for _ in range(1 + 2 + 3):      # the first checked call, the warm-up, the timed steps
        inout += inb
    idx = bench.dump_indices(count)
    assert (idx is None) == (count * 4 <= bench.DUMP_SAMPLE_BYTES)
    want = inout if idx is None else inout[idx.to(dev)]
    assert got.dtype == np.float32 and got.nbytes <= bench.DUMP_SAMPLE_BYTES
    assert got.tobytes() == want.cpu().numpy().tobytes()


@pytest.mark.gpu
def test_full_run_keeps_the_headline_and_adds_the_roofline():
    """--full (here without the extras and the CPU baseline, which have their
    own tests) carries the same headline fields plus the kernel-only figures"""
    d = _bench_n1(['--full', '--no-extras', '--no-cpu-baseline'], 1 << 22)
    for k in HEADLINE:
        assert d[k] is not None, (k, d)
    r = d['roofline']
    assert r['bound'] == 'hbm' and r['kernel_ms_avg'] > 0 and r['kernel_launches_timed'] == 30
    assert r['back_to_back']['kernel_ms_avg'] > 0
    assert set(d['config']['store_policy_xcd_mask']) == {'synchronous_entry', 'stream_ordered_entries'}


@pytest.mark.gpu
def test_plain_gpus_2_line_and_dumps(tmp_path):
    """the N > 1 plain run: the value leg alone (no parity gate, A/B, CPU
    baseline or secondary legs -- those are --full), and --dump-outputs writes
    every rank's block of the last timed call, here checked against the
    recursive-halving association regenerated on the device"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env.update(MPIX_BENCH_SAME_DEVICE='1', MPIX_BENCH_BACKEND='gloo')
    total = ((4 << 20) + 8) // 4
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2',
                        '--steps', '2', '--warmup', '1', '--rsb-bytes', str(4 * total),
                        '--dump-outputs', str(tmp_path / 'out')],
                       cwd=ROOT, capture_output=True, text=True, timeout=100, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['schedule_ran'] == 'recursive_halving', d
    assert d['metric'] == bench.METRIC_RSB and d['unit'] == 'GB/s' and d['dtype'] == 'f32', d
    assert d['value'] > 0 and d['ms_per_step'] > 0 and d['higher_is_better'] is True, d
    for k in ('parity', 'defaults_ab', 'cpu_baseline', 'reduce_local_replicas', 'roofline',
              'reduce_scatter_block_other', 'allreduce'):
        assert k not in d, k
    dev = torch.device('cuda', 0)
    for r in range(2):
        got = np.load(tmp_path / 'out' / ('reduce_scatter_block_recv_rank%d.npy' % r))
        want = bench.rh_expected_block_device(2, r, total // 2, 0x5EED0100, dev)
        assert got.dtype == np.float32 and got.tobytes() == want.cpu().numpy().tobytes(), r
