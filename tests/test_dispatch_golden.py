"""Kernel selection is what it was: the sizing queries (statistic slabs of the forward and the data gradient, weight-gradient workspace) answer
the recorded sweep of tests/golden/make_golden_dispatch.py entry for entry.  Host only: the queries launch nothing."""
import importlib.util
import os

import numpy as np

from hd_yolo_amd import _lib


def _sweep_module(golden_dir):
    spec = importlib.util.spec_from_file_location('make_golden_dispatch', os.path.join(golden_dir, 'make_golden_dispatch.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_selection_matches_recorded_sweep(golden_dir):
    mod = _sweep_module(golden_dir)
    want = np.load(os.path.join(golden_dir, 'dispatch_sweep.npz'))
    shapes = mod.shapes()
    assert np.array_equal(want['shapes'], shapes), 'the sweep grid no longer matches the recorded one'
    assert list(want['settings']) == ['='.join(map(str, s)) for s in mod.SETTINGS]
    assert len(shapes) * 8 == 374400 and len(mod.SETTINGS) == 14
    got = mod.sweep(_lib.load())
    stem_shapes = shapes[(shapes[:, 3] == 3) & (shapes[:, 5] == 6)]
    problems = []
    for key, what in (('fwd', 'hdy_conv_stat_slabs'), ('dgrad', 'hdy_conv_dgrad_stat_slabs')):
        assert got[key].shape == want[key].shape
        for i, j in np.argwhere(got[key] != want[key])[:10]:
            problems.append(f'{what}{tuple(shapes[j])} with {want["settings"][i] or "default options"}: recorded {want[key][i, j]}, now {got[key][i, j]}')
    for key, rows, stem in (('ws0', shapes, 0), ('ws1', stem_shapes, 1)):
        assert got[key].shape == want[key].shape
        for (j,) in np.argwhere(got[key] != want[key])[:10]:
            problems.append(f'hdy_conv_wgrad_workspace_bytes{tuple(rows[j]) + (stem,)}: recorded {want[key][j]}, now {got[key][j]}')
    total = sum(int((got[k] != want[k]).sum()) for k in ('fwd', 'dgrad', 'ws0', 'ws1'))
    assert total == 0, f'{total} entries differ from the recorded sweep; the first ones:\n' + '\n'.join(problems)
    # the sweep reaches every family: distinct (forward, data-gradient) answers
    assert len(np.unique(np.stack([want['fwd'], want['dgrad']], -1).reshape(-1, 2), axis=0)) >= 145


def test_weight_gradient_workspace_matches_recorded_sweep(golden_dir):
    """The workspace size is the maximum over the plans of every weight-gradient family that accepts the shape, so each family's switch and
    the generic kernel's sizing options show in it."""
    mod = _sweep_module(golden_dir)
    want = np.load(os.path.join(golden_dir, 'wgrad_sweep.npz'))
    shapes, stem_shapes = mod.shapes(), mod.wgrad_stem_shapes()
    assert np.array_equal(np.load(os.path.join(golden_dir, 'dispatch_sweep.npz'))['shapes'], shapes) and np.array_equal(want['stem_shapes'], stem_shapes), \
        'the sweep grid no longer matches the recorded one'
    assert list(want['settings']) == ['='.join(map(str, s)) for s in mod.WGRAD_SETTINGS]
    assert len(shapes) == 46800 and len(stem_shapes) == 180 and len(mod.WGRAD_SETTINGS) == 8
    # a table that has stopped seeing a family proves nothing about it: every setting moves at least one recorded answer (rows 1.. hold the
    # setting's answer minus the default one)
    for i in range(1, len(mod.WGRAD_SETTINGS)):
        moved = int((want['ws0'][i] != 0).sum() + (want['ws1'][i] != 0).sum())
        assert moved > 0, f'{want["settings"][i]} changes no recorded entry against the defaults'
    got = mod.wgrad_sweep(_lib.load())
    problems = []
    for key, rows, stem in (('ws0', shapes, 0), ('ws1', stem_shapes, 1)):
        assert got[key].shape == want[key].shape
        for i, j in np.argwhere(got[key] != want[key])[:10]:
            problems.append(f'hdy_conv_wgrad_workspace_bytes{tuple(rows[j]) + (stem,)} with {want["settings"][i] or "default options"}: '
                            f'recorded {want[key][i, j]}, now {got[key][i, j]}' + (' more than the default answer' if i else ''))
    total = sum(int((got[k] != want[k]).sum()) for k in ('ws0', 'ws1'))
    assert total == 0, f'{total} entries differ from the recorded sweep; the first ones:\n' + '\n'.join(problems)
