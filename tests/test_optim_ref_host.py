"""The float64 restatement of the optimizer step (tests/optim_ref.py) against torch.optim on float64 CPU tensors, and the host-side argument
checks of hdy_opt_step (csrc/optim.hip): every refusal is decided before a launch, so it is asked for here with made-up device addresses.
No GPU, no compute calls."""
import ctypes
import os

import numpy as np
import pytest
import torch

from hd_yolo_amd import _lib, build
from optim_ref import adam_step, ema_decay, ema_step, sgd_step

FAKE = 0x10000      # a 16-byte aligned non-NULL "device pointer": nothing below may dereference it or launch
SHAPES = [(7,), (3, 5), (4,), (6,), (2, 3), (9,)]
STEPS = 5
RTOL = 1e-12        # both sides are double and differ in operation order only: a handful of roundings of 1.1e-16, relative to the tensor's largest entry


def recipe(cls, params, **kw):
    """train.py's three groups: weight decay on the second only"""
    o = cls(params[:2], **kw)
    o.add_param_group({'params': params[2:4], 'weight_decay': 5e-3})
    o.add_param_group({'params': params[4:]})
    return o


def lr_of(step, j):
    return 0.01 * (step + 1) / 4 if j < 2 else 0.1 - 0.015 * step


def close(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    err, scale = np.abs(a - b).max(), np.abs(b).max()
    assert err <= RTOL * scale, f'{what}: error {err:.3e}, largest entry {scale:.3e}'


@pytest.mark.parametrize('name', ['SGD', 'SGD-plain', 'Adam', 'AdamW'])
def test_restatement_agrees_with_torch_in_float64(name):
    """5 steps; lr rewritten per step; parameter 3 has no gradient in steps 0-1 (its state starts at step 2, its Adam step count lags)"""
    rng = np.random.default_rng(11)
    init = [rng.standard_normal(s) for s in SHAPES]
    params = [torch.nn.Parameter(torch.tensor(a, dtype=torch.float64)) for a in init]
    if name.startswith('SGD'):
        kw = dict(lr=0.01, momentum=0.9, nesterov=True) if name == 'SGD' else dict(lr=0.01, momentum=0.8, dampening=0.1)
        opt = recipe(torch.optim.SGD, params, **kw)
        if name == 'SGD-plain':
            opt.param_groups[2]['momentum'] = 0.0           # a group without momentum keeps no buffer
    else:
        opt = recipe(getattr(torch.optim, name), params, lr=0.01, betas=(0.9, 0.99), eps=1e-8, foreach=False)
    ref_p, ref_m, ref_v, ref_n = [a.copy() for a in init], [None] * len(init), [None] * len(init), [0] * len(init)
    group_of = [0, 0, 1, 1, 2, 2]
    for step in range(STEPS):
        for j, g in enumerate(opt.param_groups):
            g['lr'] = lr_of(step, j)
        grads = [None if (i == 3 and step < 2) else rng.standard_normal(s) for i, s in enumerate(SHAPES)]
        for p, g in zip(params, grads):
            p.grad = None if g is None else torch.tensor(g, dtype=torch.float64)
        opt.step()
        for i, g in enumerate(grads):
            if g is None:
                continue
            grp = opt.param_groups[group_of[i]]
            if name.startswith('SGD'):
                ref_p[i], ref_m[i] = sgd_step(ref_p[i], g, ref_m[i], grp['lr'], grp['momentum'], grp['dampening'], grp['weight_decay'], grp['nesterov'])
            else:
                ref_n[i] += 1
                ref_p[i], ref_m[i], ref_v[i] = adam_step(ref_p[i], g, ref_m[i], ref_v[i], ref_n[i], grp['lr'], grp['betas'], grp['eps'],
                                                         grp['weight_decay'], decoupled=name == 'AdamW')
        for i, p in enumerate(params):
            close(ref_p[i], p.detach().numpy(), f'{name} step {step} parameter {i}')
            st = opt.state.get(p, {})
            if name.startswith('SGD'):
                assert (ref_m[i] is None) == (st.get('momentum_buffer') is None), (step, i)
                if ref_m[i] is not None:
                    close(ref_m[i], st['momentum_buffer'].numpy(), f'{name} step {step} buffer {i}')
            elif ref_n[i]:
                assert float(st['step']) == ref_n[i]
                close(ref_m[i], st['exp_avg'].numpy(), f'{name} step {step} exp_avg {i}')
                close(ref_v[i], st['exp_avg_sq'].numpy(), f'{name} step {step} exp_avg_sq {i}')
            else:
                assert not st
    assert ref_n[3] in (0, STEPS - 2)


def test_ema_restatement_is_the_literal_loop():
    """ModelEMA.update: v *= d; v += (1 - d) * m, with d = decay(updates)"""
    import math
    rng = np.random.default_rng(5)
    ema, ref = rng.standard_normal(100), None
    ref = ema.copy()
    for updates in range(1, 6):
        m = rng.standard_normal(100)
        d = ema_decay(updates)
        assert d == 0.9999 * (1 - math.exp(-updates / 2000))
        ema *= d
        ema += (1 - d) * m
        ref = ema_step(ref, m, d)
        close(ref, ema, f'update {updates}')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def opt_call(lib, table=FAKE, ndesc=3, blocks=3, algo=_lib.OPT_ADAMW, nesterov=0, hyper=True, nslots=2, has_ema=1):
    arr = (ctypes.c_float * (_lib.OPT_HYPER * (_lib.OPT_MAX_SLOTS + 1)))() if hyper else None
    return lib.hdy_opt_step(table, ndesc, blocks, algo, nesterov, arr, nslots, has_ema, 0.5, 0.5, None)


def test_opt_step_refuses_before_a_launch(lib):
    E = _lib.EINVAL
    err = lambda: lib.hdy_last_error().decode()
    assert opt_call(lib, table=None) == E and 'null table' in err()
    assert opt_call(lib, ndesc=0) == E and 'empty table' in err() and '0 rows' in err()
    assert opt_call(lib, blocks=0) == E and 'empty table' in err()
    assert opt_call(lib, algo=3) == E and 'unknown algorithm 3' in err()
    assert opt_call(lib, algo=-1) == E and 'unknown algorithm -1' in err()
    assert opt_call(lib, nslots=0) == E and '0 slots' in err()
    assert opt_call(lib, nslots=_lib.OPT_MAX_SLOTS + 1) == E and f'{_lib.OPT_MAX_SLOTS + 1} slots' in err()
    assert opt_call(lib, hyper=False) == E and 'null hyper-parameter array' in err()


def test_opt_abi_constants_and_descriptor(lib):
    """the binding's mirror of hdy_opt_desc and of the HDY_OPT_* constants against the header"""
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hdyolo.h')).read()
    const = lambda n: int(re.search(rf'#define\s+{n}\s+(\d+)', header).group(1))
    assert (const('HDY_OPT_SGD'), const('HDY_OPT_ADAM'), const('HDY_OPT_ADAMW')) == (_lib.OPT_SGD, _lib.OPT_ADAM, _lib.OPT_ADAMW)
    assert const('HDY_OPT_MAX_SLOTS') == _lib.OPT_MAX_SLOTS == 16 and const('HDY_OPT_HYPER') == _lib.OPT_HYPER
    assert ctypes.sizeof(_lib.OptDesc) == 64                  # five pointers, a 64-bit count, four ints
    assert lib.hdy_opt_blocks(1) == 1 and lib.hdy_opt_blocks(4096) == 1 and lib.hdy_opt_blocks(4097) == 2 and lib.hdy_opt_blocks(8196) == 3
    assert lib.hdy_exec_op(b'hdy_opt_step') >= 0
