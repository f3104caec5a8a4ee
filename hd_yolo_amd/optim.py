"""torch.optim.SGD's update as ONE HIP launch over all parameter tensors (csrc/optim.hip, `hdy_opt_step`).

Drop-in for the optimizer the reference builds (train.py:208-233: `SGD(g0, lr, momentum, nesterov=True)` + `add_param_group` for the
decayed weights and the biases; train.py:436-444 rewrites `lr` / `momentum` of every group during the warm-up; train.py:478 steps
it): same constructor arguments, `param_groups`, `state[p]['momentum_buffer']` and `state_dict()` layout, so checkpoints written with
either class load into the other.  Parameters and gradients must be contiguous fp32 CUDA tensors (the engine's gradients are views of
one flat fp32 buffer); anything else raises — there is no fallback path.

`Adam` / `AdamW` (train.py:229-231) are the same for torch.optim.Adam / AdamW, through the same launch and the same `step()`.  Every class
takes `step(ema=ModelEMA)`: the launch that writes a parameter also writes its exponential moving average (train.py:480 `ema.update(model)`
after every step; common.py:128-155), and the BatchNorm running statistics, frozen and gradient-less parameters ride along as EMA-only rows.
One launch serves `HDY_OPT_MAX_SLOTS` (16) distinct (parameter group, step count) pairs; more raise."""
import ctypes

import torch

from . import _lib


def _fp32_cuda(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)


class _Fused(torch.optim.Optimizer):
    """What the three classes share: step(), the rows, slots and cached device table of hdy_opt_step, the EMA rows, the launch.

    A subclass names its algorithm (`_algo` -> (HDY_OPT_*, nesterov), which also raises for what the class does not serve) and gives `_state_rows(group, p)` -> (m, v,
    first, step count of this step, the state dict whose 'step' follows it or None) without touching `self.state`; `_commit` makes missing
    states once every check has passed, so a refused step leaves no half-made state behind.  Host cost: while the pointers stand still a step
    is one pass over the tensors that reads their addresses, compares them with the cached table's and moves the integer step counts — no
    tensor operation per parameter."""
    _what = 'hd_yolo_amd.optim'

    def _init_fused(self):
        self._okey, self._otable, self._ondesc, self._oblocks = None, None, 0, 0
        self._ema_walk = None                 # (EMA model, model, their modules' parameter / buffer tables side by side) of the last step(ema=...)
        self.table_builds = 0                 # device tables built for hdy_opt_step so far (tests: a replaced storage must rebuild)

    def _ema_pairs(self, ema):
        """{id(model entry): (model entry, EMA entry)} over the float entries of the two state_dicts, as ModelEMA.update pairs them by name.
        The two module trees are walked side by side (the EMA model is a deep copy) and their parameter / buffer tables read directly: the
        tensors are looked up afresh in every step, so a replaced tensor or storage is seen, at a fraction of two state_dict() calls."""
        src = getattr(ema, 'src', None)
        if src is None:
            raise TypeError(f'{self._what}: step(ema=...) takes a metayolo.common.ModelEMA (its .src model is averaged into its .ema)')
        c = self._ema_walk
        if c is None or c[0] is not ema.ema or c[1] is not src:
            a, b = list(src.named_modules()), list(ema.ema.named_modules())
            if [n for n, _ in a] != [n for n, _ in b]:
                raise TypeError(f'{self._what}: the EMA model and the model it averages have different module trees')
            # the per-module tables themselves (they outlive the tensors in them), of the modules that hold anything
            c = self._ema_walk = (ema.ema, src, [(ms._parameters, me._parameters, ms._buffers, me._buffers, me._non_persistent_buffers_set)
                                                 for (_, ms), (_, me) in zip(a, b) if me._parameters or me._buffers])
        pairs = {}
        for sp, ep, sb, eb, skip in c[2]:
            for k, e in ep.items():
                if e is not None and e.dtype.is_floating_point:
                    s = sp[k]
                    pairs[id(s)] = (s, e)
            for k, e in eb.items():
                if e is not None and e.dtype.is_floating_point and k not in skip:
                    s = sb[k]
                    pairs[id(s)] = (s, e)
        return pairs

    @torch.no_grad()
    def step(self, closure=None, ema=None):
        """One step of every parameter that has a gradient; with `ema` (a ModelEMA) the same launch averages the model into it, as
        `ema.update(model)` after the step would"""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._opt_step(ema)
        return loss

    def _opt_step(self, ema):
        lib = _lib.load()
        pairs = self._ema_pairs(ema) if ema is not None else {}
        # rows: (p, g, m, v, e, slot, first, group, step count) of every table row;  key: the row's pointers, slot and `first`, what the device
        # table holds;  counts: (state dict, its new step count);  wrote: what the kernel writes, for the version counters
        rows, key, counts, slots, wrote = [], [], [], {}, []
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                m, v, first, step, st = self._state_rows(group, p)
                slot = slots.setdefault((gi, step), len(slots))
                pair = pairs.pop(id(p), None) if pairs else None
                e = None if pair is None else pair[1]
                rows.append((p, g, m, v, e, slot, first, group, step))
                key.append((p.data_ptr(), g.data_ptr(), 0 if m is None else m.data_ptr(), 0 if v is None else v.data_ptr(),
                            0 if e is None else e.data_ptr(), slot, first))
                if st is not None:
                    counts.append((st, step))
                wrote.append(p)
                if m is not None:
                    wrote.append(m)
                if v is not None:
                    wrote.append(v)
                if e is not None:
                    wrote.append(e)
        for s, e in pairs.values():               # buffers, frozen parameters, parameters without a gradient in this step
            rows.append((s, None, None, None, e, 0, False, None, 0))
            key.append((s.data_ptr(), 0, 0, 0, e.data_ptr(), 0, False))
            wrote.append(e)
        if not rows:
            return
        if len(slots) > _lib.OPT_MAX_SLOTS:
            raise ValueError(f'{self._what}: {len(slots)} distinct (parameter group, step count) pairs, one launch serves {_lib.OPT_MAX_SLOTS}')
        (algo, nesterov), dev = self._algo(), rows[0][0].device
        if key == self._okey:
            # the table of the last step serves: same tensors (checked when it was built), every state exists; only the step counts move
            for st, step in counts:
                st['step'] = step
        else:
            for p, g, m, v, e, *_ in rows:
                if not _fp32_cuda(*[t for t in (p, g, m, v, e) if t is not None]) or (e is not None and e.numel() != p.numel()):
                    raise TypeError(f'{self._what} needs contiguous fp32 CUDA parameters, gradients, states and EMA entries (of the parameter\'s size)')
            ptr = lambda t: None if t is None else t.data_ptr()
            descs, blocks, fresh = (_lib.OptDesc * len(rows))(), 0, False
            for dsc, (p, g, m, v, e, slot, first, group, step) in zip(descs, rows):
                if g is not None:
                    m, v = self._commit(group, p, m, v, step)
                    if first:
                        fresh = True
                        wrote += [t for t in (m, v) if t is not None]
                dsc.p, dsc.g, dsc.m, dsc.v, dsc.ema = ptr(p), ptr(g), ptr(m), ptr(v), ptr(e)
                dsc.n, dsc.slot, dsc.first, dsc.first_block = p.numel(), slot, int(first), blocks
                blocks += lib.hdy_opt_blocks(p.numel())
            self._otable = _lib.device_table(descs, dev)
            self._ondesc, self._oblocks = len(rows), blocks
            self.table_builds += 1
            # a table with first-step rows serves that step only (their states were made just now: the key above does not name them)
            self._okey = None if fresh else key
        nslots = max(1, len(slots))
        hyper = (ctypes.c_float * (_lib.OPT_HYPER * nslots))()
        for (gi, step), slot in slots.items():
            vals = self._hyper(self.param_groups[gi], step)
            hyper[slot * _lib.OPT_HYPER:slot * _lib.OPT_HYPER + len(vals)] = vals
        d = 0.0
        if ema is not None:
            ema.updates += 1
            d = ema.decay(ema.updates)
        rc = lib.hdy_opt_step(self._otable.data_ptr(), self._ondesc, self._oblocks, algo, int(nesterov), hyper, nslots, int(ema is not None), d, 1 - d,
                              torch.cuda.current_stream(dev).cuda_stream)
        if rc:
            raise _lib.HdyError(f'hdy_opt_step failed (status {rc}): {lib.hdy_last_error().decode()}')
        # raw-pointer writes: every `_version`-keyed cache (segrun.PackCache, ops.PackTable, ops.BnEvalTable — val.run(ema.ema) goes through them)
        # must see the parameters, the state and the EMA entries change, as after an in-place torch update
        torch._C._increment_version(wrote)


class SGD(_Fused):
    _what = 'hd_yolo_amd.optim.SGD'

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov))
        self._init_fused()

    def _algo(self):
        nesterov = {bool(g['nesterov']) for g in self.param_groups}
        if len(nesterov) != 1:
            raise ValueError('hd_yolo_amd.optim.SGD: nesterov must be the same in every parameter group')
        return _lib.OPT_SGD, nesterov.pop()

    def _state_rows(self, group, p):
        if group['momentum'] == 0:
            return None, None, False, 0, None
        buf = self.state.get(p, {}).get('momentum_buffer')
        return buf, None, buf is None, 0, None

    def _commit(self, group, p, m, v, step):
        if group['momentum'] != 0 and m is None:
            m = self.state[p]['momentum_buffer'] = torch.empty_like(p, memory_format=torch.contiguous_format)
        return m, None

    def _hyper(self, group, step):
        return [float(group[k]) for k in ('lr', 'weight_decay', 'momentum', 'dampening')]


class Adam(_Fused):
    """torch.optim.Adam (decoupled_weight_decay=True: AdamW) in one launch.  `state[p]` = {'step', 'exp_avg', 'exp_avg_sq'} as torch's, with
    `step` kept as a Python int between steps (torch keeps a CPU scalar tensor per parameter and runs a tensor operation on each of them in
    every step); `state_dict()` writes torch's tensors and `load_state_dict()` reads them, so checkpoints pass between the classes."""
    _what = 'hd_yolo_amd.optim.Adam'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f'{self._what}: invalid lr / eps / betas / weight_decay: {lr}, {eps}, {betas}, {weight_decay}')
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                                      capturable=capturable, differentiable=differentiable, fused=fused,
                                      decoupled_weight_decay=decoupled_weight_decay))
        self._unsupported()
        self._init_fused()

    def _unsupported(self):
        for group in self.param_groups:
            on = [k for k in ('amsgrad', 'maximize', 'capturable', 'differentiable') if group.get(k)]
            if on:
                raise ValueError(f'{self._what} does not support {", ".join(on)}')

    def _algo(self):
        self._unsupported()                                   # a loaded state_dict or add_param_group may have switched one on
        decoupled = {bool(g.get('decoupled_weight_decay', False)) for g in self.param_groups}
        if len(decoupled) != 1:
            raise ValueError(f'{self._what}: decoupled_weight_decay must be the same in every parameter group')
        return (_lib.OPT_ADAMW if decoupled.pop() else _lib.OPT_ADAM), False

    def _state_rows(self, group, p):
        st = self.state.get(p)
        if not st:
            return None, None, True, 1, None
        return st['exp_avg'], st['exp_avg_sq'], False, int(st['step']) + 1, st

    def _commit(self, group, p, m, v, step):
        st = self.state[p]
        st['step'] = step
        if m is None:
            m = st['exp_avg'] = torch.empty_like(p, memory_format=torch.contiguous_format)
            v = st['exp_avg_sq'] = torch.empty_like(p, memory_format=torch.contiguous_format)
        return m, v

    def _hyper(self, group, step):
        # the scalars torch.optim.adam computes in Python doubles, each rounded to float once (on the way into the ctypes array)
        lr, wd, (beta1, beta2) = float(group['lr']), float(group['weight_decay']), group['betas']
        beta1, beta2 = float(beta1), float(beta2)
        bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
        return [lr / bc1, 1 - lr * wd if group.get('decoupled_weight_decay', False) else wd, 1 - beta1, beta2, 1 - beta2, bc2 ** 0.5, float(group['eps'])]

    def state_dict(self):
        sd = super().state_dict()
        sd['state'] = {k: {n: (torch.tensor(float(x), dtype=torch.float32) if n == 'step' else x) for n, x in st.items()} for k, st in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if 'step' in st:
                st['step'] = int(st['step'])
        self._okey = None


class AdamW(Adam):
    """torch.optim.AdamW: Adam with decoupled weight decay, default 1e-2"""
    _what = 'hd_yolo_amd.optim.AdamW'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True)
