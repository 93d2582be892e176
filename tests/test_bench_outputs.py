"""bench.py's plain line and `--dump-outputs DIR`: a plain run carries the headline only (the gates, roofline, CPU
baseline and the other configurations run under --full), and writes what the timed plan computed in its last step --
the same values, plain or --full, run after run.  CPU: the checker engine through tests/bench_host_runner.py; GPU: the
real script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, 'tests', 'bench_host_runner.py')
NAMES = ('forward_output', 'backward_output')


def _bench(script, size, dump, extra=(), gpus=1, timeout=600):
    env = dict(os.environ, GFFT_DIST_BACKEND='gloo', OMP_NUM_THREADS='1')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, script, '--gpus', str(gpus), '--size', str(size), '--steps', '3', '--warmup', '1',
           '--dump-outputs', str(dump)] + list(extra)
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0]), {k: np.load(os.path.join(str(dump), k + '.npy')) for k in NAMES}


def _check_plain_line(out, size, gpus=1):
    assert out['metric'] == 'pfft_3d_c2c_%dcubed_fp64_gflops' % size and out['unit'] == 'GFLOP/s'
    assert out['higher_is_better'] is True and out['dtype'] == 'f64'
    assert out['n_gpus'] == gpus and out['steps'] == 3 and out['warmup'] == 1
    assert out['value'] > 0 and out['ms_per_step'] > 0
    for extra in ('roofline', 'hbm_copy_ceiling', 'cpu_baseline', 'other_configs', 'stages_ms', 'slab_grid'):
        assert extra not in out, extra


def _check_files(dump, arrays):
    total = sum(os.path.getsize(os.path.join(str(dump), k + '.npy')) for k in NAMES)
    assert total <= 64 << 20
    for a in arrays.values():
        assert a.dtype == np.float64 and a.ndim == 2 and a.shape[1] == 2 and np.isfinite(a).all()


def test_plain_line_and_whole_outputs_match_full_and_each_other(tmp_path):
    """16^3 is smaller than the sample: the files hold the whole arrays (row-major), so they can be checked against
    each other -- the forward output is the scaled DFT of what the step's backward returned to."""
    n = 16
    out, plain = _bench(HOST, n, tmp_path / 'plain')
    _check_plain_line(out, n)
    assert 'gates' not in out['config']
    _check_files(tmp_path / 'plain', plain)
    f = (plain['forward_output'][:, 0] + 1j * plain['forward_output'][:, 1]).reshape(n, n, n)
    b = (plain['backward_output'][:, 0] + 1j * plain['backward_output'][:, 1]).reshape(n, n, n)
    assert np.abs(b).max() > 1.0
    np.testing.assert_allclose(np.fft.fftn(b) / n ** 3, f, rtol=0, atol=1e-14 * np.abs(f).max())
    # --full gates the plan first, then times from the same seeded input: same outputs, word for word
    full, fulld = _bench(HOST, n, tmp_path / 'full', ('--full', '--no-cpu'))
    assert full['config']['exchange_check'] == 'bit-exact' and full['config']['round_trip_rel_err'] <= 1e-10
    for k in NAMES:
        assert np.array_equal(plain[k], fulld[k]), k


def test_sampled_outputs_are_the_same_run_after_run(tmp_path):
    n = 128                                          # 2^21 points per array: a seeded sample of 2^20
    out, a = _bench(HOST, n, tmp_path / 'a')
    _check_plain_line(out, n)
    _check_files(tmp_path / 'a', a)
    assert all(x.shape == (1 << 20, 2) for x in a.values())
    _, b = _bench(HOST, n, tmp_path / 'b')
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k


def test_two_ranks_dump_both_blocks(tmp_path):
    n = 32
    out, a = _bench(HOST, n, tmp_path / 'a', gpus=2)
    _check_plain_line(out, n, gpus=2)
    assert out['config']['exchange_check'] == 'bit-exact'       # at N > 1 the plans are gated in every run
    _check_files(tmp_path / 'a', a)
    assert all(x.shape == (n ** 3, 2) for x in a.values())      # two blocks of n^3 / 2, rank 0's first
    _, b = _bench(HOST, n, tmp_path / 'b', gpus=2)
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
def test_gpu_plain_line_and_outputs_match_full(tmp_path):
    n = 128
    out, plain = _bench(os.path.join(ROOT, 'bench.py'), n, tmp_path / 'plain')
    _check_plain_line(out, n)
    _check_files(tmp_path / 'plain', plain)
    assert all(x.shape == (1 << 20, 2) for x in plain.values())
    assert np.abs(plain['backward_output']).max() > 1.0
    full, fulld = _bench(os.path.join(ROOT, 'bench.py'), n, tmp_path / 'full', ('--full', '--no-cpu'))
    assert full['roofline']['frac'] > 0 and full['config']['forward_rel_err'] <= 2e-10
    for k in NAMES:
        assert np.array_equal(plain[k], fulld[k]), k
