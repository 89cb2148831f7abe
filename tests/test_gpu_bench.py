"""GPU: bench.py times exactly --steps steps (a remainder call when --steps is not a multiple of the 20 jobs per call) and
--dump-outputs writes what the last timed step returned: its 1000 scores and its stable top-100."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_bench_exact_steps_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / 'dump'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '47', '--warmup', '5', '--no-cpu-baseline',
           '--no-probes', '--dump-outputs', str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    assert j['steps'] == 47 and j['calls'] == 3
    assert j['ms_per_step'] > 0 and j['ms_per_step'] == pytest.approx(j['timed_region_ms'] / 47)
    assert j['value'] == pytest.approx(47 * 1000 / (j['timed_region_ms'] * 1e-3))
    scores = np.load(out_dir / 'scores.npy')
    top_s = np.load(out_dir / 'top_scores.npy')
    top_i = np.load(out_dir / 'top_indices.npy')
    assert scores.dtype == np.float32 and scores.shape == (1000,) and np.isfinite(scores).all()
    assert top_s.dtype == np.float32 and top_s.shape == (100,)
    assert top_i.dtype == np.float64 and top_i.shape == (100,)
    order = np.argsort(-scores, kind='stable')[:100]          # evaluate.py:76: stable descending sort
    assert np.array_equal(top_i, order.astype(np.float64)) and np.array_equal(top_s, scores[order])


@pytest.mark.timeout(600)
def test_bench_plain_run_is_the_headline_alone():
    """A plain run prints the headline fields and none of the side measurements; --full adds them to the same fields."""
    def run(*extra):
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '40', '--warmup', '5', *extra]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        return json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    plain = run()
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in plain
    assert plain['steps'] == 40 and plain['calls'] == 2 and plain['value'] > 0 and plain['higher_is_better'] is True
    assert not {'roofline', 'one_stream', 'single_job', 'config3', 'config4', 'e2e', 'cpu_baseline', 'rccl'} & set(plain)
    full = run('--full', '--no-cpu-baseline', '--no-probes')
    assert set(plain) <= set(full) and full['metric'] == plain['metric'] and full['unit'] == plain['unit']
    assert full['one_stream']['value'] > 0 and full['single_job']['us_per_call'] > 0 and full['roofline']['kernel_ms'] > 0
