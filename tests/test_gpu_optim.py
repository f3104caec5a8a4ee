"""hd_yolo_amd.optim.SGD / Adam / AdamW, step() and step(ema=...) (csrc/optim.hip, hdy_opt_step) on a real MI355X, against the float64
restatement of tests/optim_ref.py, with torch.optim on the GPU as the yardstick for what fp32 can give.

Shapes: lengths 1, 3, 4, 5 (scalar tail), 4095 / 4096 / 4097 (block boundary), 8196 (three blocks, a partial last one), a (64, 32, 3, 3)
filter, a 4100-element view at storage offset 1 (4-byte aligned only: scalar path although n % 4 == 0) and a parameter that gets its first
gradient in step 2 (two step counts in one group: two slots).  Three parameter groups as train.py builds them, weight decay on the second,
lr (and SGD's momentum) rewritten before every step."""
import copy
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hd_yolo_amd import _lib  # noqa: E402
from hd_yolo_amd.optim import SGD, Adam, AdamW  # noqa: E402
from metayolo.common import ModelEMA  # noqa: E402
from optim_ref import adam_step, ema_decay, ema_step  # noqa: E402

DEV = 'cuda:0'
EPS32 = 2.0 ** -23
SHAPES = [(1,), (3,), (4,), (5,), (4095,), (4096,), (4097,), (8196,), (64, 32, 3, 3)]
VIEW, LATE = 9, 10                                   # the offset-1 view, the parameter that joins in step 2
GROUPS = ([0, 1, 2, 8], [3, 4, 5, VIEW, LATE], [6, 7])
FUSED = {'SGD': SGD, 'Adam': Adam, 'AdamW': AdamW}
KW = {'SGD': dict(lr=0.01, momentum=0.9, nesterov=True), 'Adam': dict(lr=0.01, betas=(0.9, 0.99)), 'AdamW': dict(lr=0.01, betas=(0.9, 0.99))}


def f64(t):
    return None if t is None else t.detach().double().cpu().numpy()


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


class Bag(torch.nn.Module):
    """the parameter set above; convs: two Conv(8, 8, 3) blocks (BatchNorm buffers); idle: a frozen parameter and one that never gets a gradient"""

    def __init__(self, convs=False, idle=False):
        super().__init__()
        ps = [torch.nn.Parameter(randn(s, i)) for i, s in enumerate(SHAPES)]
        view = torch.nn.Parameter(randn((4101,), 50)[1:])
        assert view.data_ptr() % 16 == 4 and view.numel() % 4 == 0 and view.is_contiguous()
        ps += [view, torch.nn.Parameter(randn((37,), 51))]
        self.ps = torch.nn.ParameterList(ps)
        if convs:
            from metayolo.models.layers import Conv
            torch.manual_seed(3)
            self.c1, self.c2 = Conv(8, 8, 3).to(DEV), Conv(8, 8, 3).to(DEV)
        if idle:
            self.frozen = torch.nn.Parameter(randn((40,), 52), requires_grad=False)
            self.unused = torch.nn.Parameter(randn((4100,), 53))

    def trained(self):
        return list(self.ps) + ([p for c in (self.c1, self.c2) for p in c.parameters()] if hasattr(self, 'c1') else [])


def make_opt(cls, bag, **kw):
    ps = list(bag.ps)
    g0 = [ps[i] for i in GROUPS[0]] + bag.trained()[len(ps):] + ([bag.frozen, bag.unused] if hasattr(bag, 'frozen') else [])
    o = cls(g0, **kw)
    o.add_param_group({'params': [ps[i] for i in GROUPS[1]], 'weight_decay': 5e-3})
    o.add_param_group({'params': [ps[i] for i in GROUPS[2]]})
    if 'momentum' in kw:
        o.param_groups[2]['momentum'] = 0.0                 # a group without momentum: no buffer
    return o


def warm_up(opt, step):
    for j, g in enumerate(opt.param_groups):
        g['lr'] = 0.01 * (step + 1) / 4 if j < 2 else 0.1 - 0.015 * step
        if g.get('momentum'):
            g['momentum'] = 0.8 + 0.03 * step


def set_grads(bag, step, late=True):
    """new values in the same gradient tensors, as the engine's flat gradient buffer gives: the device table is keyed on the pointers"""
    for i, p in enumerate(bag.trained()):
        if late and i == LATE and step < 2:
            p.grad = None
        elif p.grad is None:
            p.grad = randn(p.shape, 1000 + 100 * step + i)
        else:
            p.grad.copy_(randn(p.shape, 1000 + 100 * step + i))


def step_errors(opt, params, decoupled, **step_kw):
    """One step of an Adam-family optimizer; -> (largest |error| against the float64 restatement fed with the fp32 states and gradients the
    step started from, largest |reference|), each pooled over all tensors, for p, exp_avg and exp_avg_sq."""
    group_of = {id(p): g for g in opt.param_groups for p in g['params']}
    snap = []
    for p in params:
        st = opt.state.get(p) or {}
        snap.append((f64(p), f64(st.get('exp_avg')), f64(st.get('exp_avg_sq')), int(float(st.get('step', 0))), f64(p.grad)))
    opt.step(**step_kw)
    names = ('p', 'exp_avg', 'exp_avg_sq')
    err, scale = dict.fromkeys(names, 0.0), dict.fromkeys(names, 0.0)
    for p, (p0, m0, v0, n, g) in zip(params, snap):
        if g is None:
            assert np.array_equal(f64(p), p0) and int(float((opt.state.get(p) or {}).get('step', 0))) == n
            continue
        grp = group_of[id(p)]
        ref = adam_step(p0, g, m0, v0, n + 1, grp['lr'], grp['betas'], grp['eps'], grp['weight_decay'], decoupled)
        st = opt.state[p]
        assert float(st['step']) == n + 1
        for name, got, r in zip(names, (p, st['exp_avg'], st['exp_avg_sq']), ref):
            err[name] = max(err[name], float(np.abs(f64(got) - r).max()))
            scale[name] = max(scale[name], float(np.abs(r).max()))
    return err, scale


def assert_as_good_as_torch(ef, et, scale, what):
    """e_fused <= 2 * e_torch + eps32 * max|x|: twice torch's own error for an equally valid rounding order, the floor for where torch is exact"""
    for name in ef:
        print(f'{what} {name}: fused {ef[name]:.3e} torch {et[name]:.3e} max|x| {scale[name]:.3e}')
        assert ef[name] <= 2 * et[name] + EPS32 * scale[name], f'{what} {name}: fused error {ef[name]:.3e}, torch error {et[name]:.3e}, max|x| {scale[name]:.3e}'


@pytest.mark.parametrize('name', ['Adam', 'AdamW'])
def test_adam_is_as_close_to_float64_as_torch(name):
    bf, bt = Bag(), Bag()
    of, ot = make_opt(FUSED[name], bf, **KW[name]), make_opt(getattr(torch.optim, name), bt, **KW[name])
    for step in range(5):
        warm_up(of, step), warm_up(ot, step)
        set_grads(bf, step)
        with torch.no_grad():
            for a, b in zip(bf.ps, bt.ps):                  # torch starts every step from the fused side's fp32 state
                b.copy_(a)
                b.grad = None if a.grad is None else a.grad.clone()
                st = of.state.get(a)
                if st:
                    ot.state[b] = {'step': torch.tensor(float(st['step'])), 'exp_avg': st['exp_avg'].clone(), 'exp_avg_sq': st['exp_avg_sq'].clone()}
        ef, scale = step_errors(of, list(bf.ps), name == 'AdamW')
        et, _ = step_errors(ot, list(bt.ps), name == 'AdamW')
        assert_as_good_as_torch(ef, et, scale, f'{name} step {step}')
        for a, b in zip(bf.ps, bt.ps):
            sa, sb = of.state.get(a), ot.state.get(b)
            assert bool(sa) == bool(sb) and (not sa or float(sa['step']) == float(sb['step'])), step
    assert of.state[bf.ps[LATE]]['step'] == 3 and of.state[bf.ps[0]]['step'] == 5


def sha256(tensors):
    """one SHA-256 over the raw fp32 bytes of the tensors, in order"""
    h = hashlib.sha256()
    for t in tensors:
        assert t.dtype == torch.float32
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def sgd_bits(with_ema=False):
    """Four SGD steps of the recipe above, as digests: {'initial_parameters', 'steps': [{'gradients', 'parameters': one per tensor of bag.ps,
    'momentum_buffers': one per tensor, None where it has none}]}.  tests/golden/make_golden_optim_sgd.py recorded optim_sgd_bits.json with it."""
    bag = Bag()
    opt = make_opt(SGD, bag, **KW['SGD'])
    step_kw = {'ema': ModelEMA(bag)} if with_ema else {}
    out = {'initial_parameters': sha256(bag.ps), 'steps': []}
    for step in range(4):
        warm_up(opt, step)
        set_grads(bag, step)
        grads = sha256([p.grad for p in bag.ps if p.grad is not None])
        opt.step(**step_kw)
        bufs = [opt.state.get(p, {}).get('momentum_buffer') for p in bag.ps]
        out['steps'].append({'gradients': grads, 'parameters': [sha256([p]) for p in bag.ps],
                             'momentum_buffers': [None if b is None else sha256([b]) for b in bufs]})
    return out


def test_sgd_bits_are_those_of_the_retired_kernel():
    """SGD.step() gives, bit for bit, what the SGD-only `sgd_step_kernel` (retired with ABI revision 15) gave on the same recipe at the last
    commit that had it: tests/golden/optim_sgd_bits.json, written there by tests/golden/make_golden_optim_sgd.py"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'optim_sgd_bits.json')) as f:
        want = json.load(f)
    got = sgd_bits()
    assert len(got['steps']) == len(want['steps']) == 4
    inputs = lambda bits: [bits['initial_parameters']] + [s['gradients'] for s in bits['steps']]
    assert inputs(got) == inputs(want), 'the inputs no longer reproduce (initial parameters or gradients of the recipe): this says nothing about the update'
    for step, (g, w) in enumerate(zip(got['steps'], want['steps'])):
        assert len(g['parameters']) == len(w['parameters']) == len(SHAPES) + 2
        for i, (a, b) in enumerate(zip(g['parameters'], w['parameters'])):
            assert a == b, f'step {step}: parameter {i} differs from the retired kernel\'s'
        for i, (a, b) in enumerate(zip(g['momentum_buffers'], w['momentum_buffers'])):
            assert (b is None) == (i in GROUPS[2] or (i == LATE and step < 2)), (step, i)
            assert a == b, f'step {step}: momentum buffer {i} differs from the retired kernel\'s'


@pytest.mark.parametrize('name', ['SGD', 'Adam', 'AdamW'])
def test_the_ema_does_not_change_the_update(name):
    """rank 0 steps with the EMA, the other ranks without (train.py): their parameters and states must stay the same bits"""
    ba, bb = Bag(), Bag()
    oa, ob = make_opt(FUSED[name], ba, **KW[name]), make_opt(FUSED[name], bb, **KW[name])
    ema = ModelEMA(bb)
    for step in range(4):
        warm_up(oa, step), warm_up(ob, step)
        set_grads(ba, step), set_grads(bb, step)
        oa.step()
        ob.step(ema=ema)
        for i, (a, b) in enumerate(zip(ba.ps, bb.ps)):
            assert torch.equal(a, b), (step, i)
            sa, sb = oa.state.get(a), ob.state.get(b)
            assert bool(sa) == bool(sb), (step, i)
            if sa:
                assert list(sa) == list(sb), (step, i)
                for k, x in sa.items():
                    assert torch.equal(x, sb[k]) if torch.is_tensor(x) else x == sb[k], (step, i, k)
            if name == 'SGD':                                 # no buffer for the momentum-free group, nor for the late parameter before step 2
                assert (not sa) == (i in GROUPS[2] or (i == LATE and step < 2)), (step, i)
                assert not sa or list(sa) == ['momentum_buffer']
    assert oa.table_builds > 0 and ob.table_builds > 0


def ema_snapshot(ema):
    return {k: v.clone() for k, v in ema.ema.state_dict().items()}


def check_ema(before, ema, d, what):
    """every float entry of ema.ema against d * before + (1 - d) * (the model's fp32 entry as it stands), within 4 eps32 (|d*ema| + |(1-d)*p|):
    either form of the sum has at most two roundings per term; integer entries untouched"""
    msd = ema.src.state_dict()
    for k, e in ema.ema.state_dict().items():
        if not e.dtype.is_floating_point:
            assert torch.equal(e, before[k]), (what, k)
            continue
        e0, p = f64(before[k]), f64(msd[k])
        bound = 4 * EPS32 * (np.abs(d * e0) + np.abs((1 - d) * p))
        over = np.abs(f64(e) - ema_step(e0, p, d)) - bound
        assert over.max() <= 0, f'{what} {k}: {over.max():.3e} beyond the bound'


def perturb_buffers(bag, step):
    with torch.no_grad():
        for j, c in enumerate((bag.c1, bag.c2)):
            c.bn.running_mean.add_(0.1 * randn(c.bn.running_mean.shape, 70 + 10 * step + j))
            c.bn.running_var.mul_(1.0 + 0.1 * (step + 1))
            c.bn.num_batches_tracked.add_(1)


@pytest.mark.parametrize('name', ['SGD', 'Adam', 'AdamW'])
def test_ema_values_after_each_fused_step(name):
    bag = Bag(convs=True)
    opt = make_opt(FUSED[name], bag, **KW[name])
    ema = ModelEMA(bag)
    with torch.no_grad():
        for c in (ema.ema.c1, ema.ema.c2):
            c.bn.num_batches_tracked.fill_(7)
    for step in range(4):
        warm_up(opt, step)
        set_grads(bag, step)
        perturb_buffers(bag, step)
        before = ema_snapshot(ema)
        opt.step(ema=ema)
        assert ema.updates == step + 1
        d = ema.decay(ema.updates)
        assert d == ema_decay(step + 1)
        check_ema(before, ema, d, f'{name} step {step}')
        after = ema.ema.state_dict()
        for k in ('c1.bn.running_mean', 'c1.bn.running_var', 'c2.bn.running_mean', 'c2.bn.running_var', 'c2.conv.weight', 'ps.0', f'ps.{VIEW}'):
            assert not torch.equal(after[k], before[k]), (step, k)
        assert int(after['c1.bn.num_batches_tracked']) == 7 and int(bag.c1.bn.num_batches_tracked) == step + 1


@pytest.mark.parametrize('name', ['SGD', 'AdamW'])
def test_ema_only_rows_leave_the_parameter_alone(name):
    bag = Bag(idle=True)
    opt = make_opt(FUSED[name], bag, **KW[name])
    ema = ModelEMA(bag)
    p0 = {k: getattr(bag, k).detach().clone() for k in ('frozen', 'unused')}
    for step in range(2):
        set_grads(bag, step)
        before = ema_snapshot(ema)
        opt.step(ema=ema)
        check_ema(before, ema, ema.decay(ema.updates), f'{name} step {step}')
        for k, was in p0.items():
            p = getattr(bag, k)
            assert torch.equal(p, was) and p not in opt.state, k
            assert not torch.equal(ema.ema.state_dict()[k], before[k]), k
        assert bag.ps[LATE] not in opt.state                  # no gradient yet: an EMA-only row as well


@pytest.mark.parametrize('how', ['half_float', 'load_assign', 'load_in_place'])
def test_replaced_ema_storage_is_followed(how):
    bag = Bag(convs=True)
    opt = make_opt(AdamW, bag, **KW['AdamW'])
    ema = ModelEMA(bag)
    for step in range(3):                                     # the first step's table is good for that step only; the second one's is kept
        set_grads(bag, step, late=False)
        opt.step(ema=ema)
    assert opt.table_builds == 2
    old = {k: v.data_ptr() for k, v in ema.ema.state_dict().items()}
    if how == 'half_float':
        ema.ema.half().float()                                # train.py:230-231 around the validation of a plain torch module
    else:
        sd = {k: (v.clone() * 0.5 if v.dtype.is_floating_point else v.clone()) for k, v in ema.ema.state_dict().items()}
        ema.ema.load_state_dict(sd, assign=how == 'load_assign')
    moved = [k for k, v in ema.ema.state_dict().items() if v.data_ptr() != old[k]]
    assert (len(moved) > 0) == (how != 'load_in_place')
    set_grads(bag, 3, late=False)
    before = ema_snapshot(ema)
    opt.step(ema=ema)
    check_ema(before, ema, ema.decay(ema.updates), how)
    assert ema.updates == 4 and opt.table_builds == (2 if how == 'load_in_place' else 3)


def test_versions_move_and_the_engine_sees_the_new_ema():
    bag = Bag(convs=True)
    opt = make_opt(AdamW, bag, **KW['AdamW'])
    ema = ModelEMA(bag)
    set_grads(bag, 0, late=False)
    opt.step(ema=ema)
    set_grads(bag, 1, late=False)
    watched = bag.trained() + [opt.state[p][k] for p in bag.trained() for k in ('exp_avg', 'exp_avg_sq')] + \
        [v for v in ema.ema.state_dict(keep_vars=True).values() if v.dtype.is_floating_point]
    was = [t._version for t in watched]
    opt.step(ema=ema)
    assert all(t._version > v for t, v in zip(watched, was))

    # the engine's packed weights and folded BatchNorm coefficients are keyed on _version: a second forward of the SAME ema.ema object must
    # see the step (B), as a fresh model loaded from its state_dict does (C), and not repeat the first forward (A)
    from hd_yolo_amd import synth
    from test_gpu_kernels import TOL, assert_close
    from test_gpu_model import build
    model = build('n', 2)
    ema = ModelEMA(model)
    x = synth.synth_images(2, 64, seed=7).to(DEV)

    def forward(m):
        with torch.no_grad():
            plan = m._eng().plan_for(x, False, torch.float32)
            plan.run_forward(x)
            return plan.feature(9).clone()
    a = forward(ema.ema)
    opt = AdamW(model.parameters(), lr=0.05)
    for i, p in enumerate(model.parameters()):
        p.grad = randn(p.shape, 2000 + i)
    opt.step(ema=ema)
    b = forward(ema.ema)
    fresh = build('n', 2).eval()
    fresh.load_state_dict(ema.ema.state_dict())
    c = forward(fresh)
    assert_close(b, c, TOL[torch.float32], 'second forward of ema.ema against a fresh model with its state')
    assert (b - a).abs().max() > 1e-3 * a.abs().max()


@pytest.mark.parametrize('name', ['Adam', 'AdamW'])
@pytest.mark.parametrize('direction', ['fused_to_torch', 'torch_to_fused'])
def test_checkpoints_pass_between_the_classes(name, direction):
    tcls, decoupled = getattr(torch.optim, name), name == 'AdamW'
    first, second = (FUSED[name], tcls) if direction == 'fused_to_torch' else (tcls, FUSED[name])
    ba, bb = Bag(), Bag()
    oa = make_opt(first, ba, **KW[name])
    for step in range(3):
        warm_up(oa, step)
        set_grads(ba, step)
        oa.step()
    sd = oa.state_dict()
    assert all(torch.is_tensor(s['step']) and s['step'].dtype == torch.float32 and list(s) == ['step', 'exp_avg', 'exp_avg_sq'] for s in sd['state'].values())
    assert sorted(sd['param_groups'][0]) == sorted(make_opt(tcls, Bag(), **KW[name]).state_dict()['param_groups'][0])
    ob = make_opt(second, bb, **KW[name])
    with torch.no_grad():
        for a, b in zip(ba.ps, bb.ps):
            b.copy_(a)
    ob.load_state_dict(copy.deepcopy(sd))
    of, bf, ot, bt = (oa, ba, ob, bb) if direction == 'fused_to_torch' else (ob, bb, oa, ba)
    for step in range(3, 5):
        warm_up(of, step), warm_up(ot, step)
        set_grads(bf, step), set_grads(bt, step)
        ef, scale = step_errors(of, list(bf.ps), decoupled)
        et, _ = step_errors(ot, list(bt.ps), decoupled)
        assert_as_good_as_torch(ef, et, scale, f'{name} {direction} step {step}')
    for a, b in zip(bf.ps, bt.ps):
        assert float(of.state[a]['step']) == float(ot.state[b]['step'])
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_what_is_not_served_raises():
    p = torch.nn.Parameter(torch.zeros(4, device=DEV))
    for cls in (Adam, AdamW):
        for k in ('amsgrad', 'maximize', 'capturable', 'differentiable'):
            with pytest.raises(ValueError, match=k):
                cls([p], **{k: True})
    for bad in (torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))):
        bad.grad = torch.zeros_like(bad)
        for cls, kw in ((Adam, {}), (AdamW, {}), (SGD, {}), (SGD, dict(momentum=0.9))):
            opt = cls([bad], **kw)
            with pytest.raises(TypeError):
                opt.step()
            assert not opt.state
    many = [torch.nn.Parameter(torch.zeros(4, device=DEV)) for _ in range(_lib.OPT_MAX_SLOTS + 1)]
    for q in many:
        q.grad = torch.ones_like(q)
    for cls, kw in ((AdamW, {}), (SGD, dict(lr=0.1)), (SGD, dict(lr=0.1, momentum=0.9))):
        opt = cls([{'params': [q]} for q in many], **kw)
        with pytest.raises(ValueError, match='17 distinct'):
            opt.step()
        assert not opt.state and all(float(q.detach().sum()) == 0 for q in many)      # refused before anything was made or written
    with pytest.raises(TypeError, match='ModelEMA'):
        AdamW([p]).step(ema=object())


def repeat_runs(name, with_ema):
    runs = []
    for _ in range(2):
        bag = Bag(convs=True)
        opt = make_opt(FUSED[name], bag, **KW[name])
        ema = ModelEMA(bag)
        for step in range(3):
            warm_up(opt, step)
            set_grads(bag, step)
            opt.step(ema=ema if with_ema else None)
        out = [p.detach().clone() for p in bag.trained()] + [v.clone() for v in ema.ema.state_dict().values()]
        out += [t.clone() for p in bag.trained() for t in opt.state.get(p, {}).values() if torch.is_tensor(t)]
        runs.append(out)
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize('name', ['SGD', 'Adam', 'AdamW'])
def test_repeats_are_bit_identical(name):
    repeat_runs(name, True)


@pytest.mark.parametrize('name', ['SGD', 'Adam', 'AdamW'])
def test_repeats_without_the_ema_are_bit_identical(name):
    repeat_runs(name, False)
