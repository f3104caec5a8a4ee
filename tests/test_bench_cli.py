"""bench.py's launcher contract on a box without a GPU: `--gpus N` with no rendezvous in the environment starts its own ranks
(torch.distributed.run on 127.0.0.1, free port) BEFORE torch is imported, and a failing rank's exit status comes back as bench.py's own —
here every rank fails at once, loudly, because the product path has no CPU fallback."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)         # __name__ != '__main__': nothing is spawned or run
    return mod


def test_gpus_flag_is_parsed_before_torch_is_imported():
    b = _load_bench()
    assert b._requested_gpus(['--steps', '3']) == 1
    assert b._requested_gpus(['--gpus', '8', '--steps', '3']) == 8
    assert b._requested_gpus(['--steps', '3', '--gpus=4']) == 4


@pytest.mark.timeout(300)
def test_a_failing_rank_fails_the_launcher():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is visible: the ranks would run (tests/test_gpu_entrypoints.py covers that side)')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, 'bench.py', '--gpus', '2', '--steps', '1', '--warmup', '0', '--no-roofline', '--no-cpu-baseline', '--no-infer'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode != 0, 'two ranks without a GPU must not report success'
    assert 'no MI355X visible' in p.stderr and 'rank 1' in p.stderr, p.stderr[-3000:]
    assert not [l for l in p.stdout.splitlines() if l.startswith('{')], 'no JSON line from a failed run'


def test_dump_outputs_writes_float32_and_samples_the_same_elements_above_the_budget(tmp_path):
    """--dump-outputs' writer (no GPU needed): one float32 .npy per loss term, parameter and floating buffer; within the budget the arrays
    are whole, above it every tensor keeps the same share of its elements at the same seeded indices on every call."""
    import numpy as np
    import torch
    b = _load_bench()
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 3), torch.nn.BatchNorm2d(16), torch.nn.Conv2d(16, 64, 3))
    losses = {'det': {'det_loss': torch.tensor(1.5), 'loss_items': {'box': torch.tensor(0.25, dtype=torch.float64)}}}
    n, frac = b.dump_outputs(str(tmp_path / 'whole'), losses, model)
    got = {f.name[:-4]: np.load(f) for f in (tmp_path / 'whole').glob('*.npy')}
    assert frac == 1.0 and n == len(got) == 2 + 6 + 2            # 2 loss terms, 6 parameters, running mean and variance
    assert sorted(got) == sorted(['loss.det.det_loss', 'loss.det.loss_items.box'] + ['param.' + k for k, _ in model.named_parameters()]
                                 + ['buffer.' + k for k, v in model.named_buffers() if v.is_floating_point()])
    assert all(v.dtype == np.float32 for v in got.values())
    np.testing.assert_array_equal(got['param.2.weight'], model[2].weight.detach().numpy())
    assert float(got['loss.det.loss_items.box']) == 0.25
    b.DUMP_BUDGET_BYTES = 4 * 1000                               # far below the model's 10 k elements
    runs = []
    for d in ('s1', 's2'):
        _, frac = b.dump_outputs(str(tmp_path / d), losses, model)
        runs.append({f.name[:-4]: np.load(f) for f in (tmp_path / d).glob('*.npy')})
    assert frac < 1.0 and sum(v.size for v in runs[0].values()) <= 1000 + len(runs[0])
    w = model[2].weight.detach().numpy().reshape(-1)
    s = runs[0]['param.2.weight']
    assert 0 < s.size < w.size and np.isin(s, w).all()
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k])
