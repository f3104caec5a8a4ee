"""Static execution plan for the metayolo backbone + neck + detection convs on MI355X.

The reference runs the network as ~200 eager ATen calls per forward plus autograd's dynamic graph
(metayolo/models/yolov5.py:53-59, :68-77; layers.py:37-38; train.py:457,472).  Here the module tree is traced
ONCE per (input shape, arithmetic type, train/eval) into a flat list of kernel launches over pre-allocated
NHWC buffers; forward and backward are replays of two launch lists.  What the tracing decides:

  * layout      activations NHWC bf16/fp32 in HBM, never NCHW; torch.cat along C is free: every producer writes
                straight into its channel slice of the concat buffer (pixel pitch = concat width).
  * fusion      C3's cv1 and cv2 (two 1x1 convs on the same input) become ONE conv with K = 2c_ (train mode);
                BN statistics come out of the conv kernel's epilogue as per-tile slabs; normalise+SiLU(+residual)
                is one streaming pass; in eval mode BN is folded into the conv epilogue (scale/shift/SiLU/residual).
  * forward     replay in trace order: one emitter per unit kind (_fwd_conv / _fwd_pool / _fwd_up / _fwd_det) appends to the
                record list.  An eval ConvUnit is one launch (BN through the bn_eval table, or the bias of a BN-folded model); a
                training ConvUnit's BatchNorm forward is _bn_fwd_mode(u) ('sync' / 'pair' / 'single' / 'frozen'): one
                _bn_fwd_<mode> emitter each, all ending in the one apply pass _bn_fwd_apply.  A unit's geometry (hin, win, M,
                pack kind, stem_hw) is fixed when it is traced.
  * memory      _allocate: activation storage; per-unit buffers, one allocator per unit kind (_alloc_conv / _alloc_det /
                _alloc_pool), each telling a _Scratch what the shared scratch buffers must hold; those buffers; gradient
                storage, which mirrors activation storage (concat members share, a shortcut input aliases the block output).
  * backward    reverse replay: [BN+SiLU backward -> dy] -> wgrad -> dgrad, gradients of multiply-consumed tensors are
                accumulated in the dgrad epilogue (no add kernels); the Bottleneck shortcut aliases gradient storage.
                _mark_needs_grad says which tensors get a gradient, then one emitter per unit kind (_bwd_det / _bwd_up /
                _bwd_pool / _bwd_conv) appends to a _BackwardList (records, fork tokens, dy ring slots, who wrote a gradient
                last, which record writes which parameter's).  A ConvUnit's BatchNorm backward is (consumer, statistics
                mode) = _bn_bwd_mode(u): one _bn_bwd_<mode> emitter each; the consumer picks the gradient launches.
  * gradients   all parameter gradients live in one flat fp32 buffer (views per parameter) so data-parallel
                all-reduce is a few large RCCL calls (hd_yolo_amd/parallel.py).

torch is used for memory (torch.empty), streams and the autograd hook-in (one custom Function around the whole
plan); every arithmetic op inside is a HIP kernel from libhdyolo_hip.so.
"""
import os

import torch
import torch.nn as nn

from . import _lib, ops

USE_GRAPHS = os.environ.get('HDY_GRAPH', '0') == '1'   # hipGraph replay of ~400-node graphs measured slower than eager on ROCm 7.2
SIDE_WGRAD = os.environ.get('HDY_SIDE_WGRAD', '1') == '1' and not USE_GRAPHS      # weight gradients on a second stream
DY_RING = int(os.environ.get('HDY_DY_RING', '4'))
SKIP_WGRAD = os.environ.get('HDY_SKIP_WGRAD') == '1'     # measurement only: no weight-gradient launches at all
# BN-backward reduce pass served by the launch that completes dz ('1': fused 1x1 backward and dgrad launches, 'fused': the former only).
# Built, parity-tested (tests/test_gpu_kernels.py, test_gpu_model.py) and NOT the default: the epilogues that would serve the statistics are
# themselves VALU-bound (exp + rcp per element on top of the store loop) — yolov5s B=64 step 14.09 ms without, 14.31 ('fused'), 14.37 ('1').
PRODUCER_STATS = os.environ.get('HDY_PRODUCER_STATS', 'fused')       # 'fused': statistics served by the fused 1x1 backward kernel only (train step 13.47 vs 13.54 ms off); '1': by dgrad epilogues too (slower); '0': off
STEM_FUSED = os.environ.get('HDY_STEM_FUSED', '1') == '1'   # the stem's weight gradient applies its unit's BatchNorm / SiLU backward itself (no dy tensor)
FUSED_1X1 = os.environ.get('HDY_FUSED_1X1', '1') == '1'     # BN-apply + wgrad + dgrad of eligible 1x1 units in one kernel (conv1x1_bwd.hip)
# probe, off: the weight re-pack on a second stream beside the input conversion (both are needed in front of the first convolution, neither depends on
# the other).  Measured round 5, one box, alternating x3: 11.813 / 11.799 / 11.793 ms per step with it, 11.673 / 11.665 / 11.649 without — the two
# cross-stream dependencies cost the main queue more than the 50-us gather they hide
PACK_SIDE = os.environ.get('HDY_PACK_SIDE', '0') == '1'
FORK_MIN_PIXELS = int(os.environ.get('HDY_FORK_MIN_PIXELS', '0'))     # probe: weight gradients of layers with fewer output pixels run inline on the main stream (no fork marker)
GRAD_BUCKET_BYTES = int(os.environ.get('HDY_GRAD_BUCKET_MB', '6')) << 20      # granularity of the "these gradients are final" marks


class Val:
    """A tensor of the traced graph: logical NHWC shape + where it lives (buffer, channel offset)."""
    __slots__ = ('n', 'h', 'w', 'c', 'name', 'buf', 'off', 'cat', 'parts', 'gbuf', 'goff', 'ginit', 'galias', 'gfinal',
                 'order', 'last_use', 'index', 'needs_grad')

    def __init__(self, n, h, w, c, name, order):
        self.n, self.h, self.w, self.c, self.name, self.order = n, h, w, c, name, order
        self.buf = self.gbuf = self.cat = self.galias = self.gfinal = None
        self.off = self.goff = 0
        self.parts = None          # for concat values: [(Val, offset)]
        self.ginit = False
        self.last_use = order
        self.index = None          # model-level node index, when this is a layer output
        self.needs_grad = True     # False: nothing trainable upstream (Model.freeze): no gradient is propagated into it

    def t(self):
        return self.buf[..., self.off:self.off + self.c]

    def g(self):
        return self.gbuf[..., self.goff:self.goff + self.c]

    def gread(self):
        return self.gfinal if self.gfinal is not None else self.g()


class ConvUnit:
    def __init__(self, mods, x, res, outs, stem, hin, win):
        """hin, win: the extent the convolution reads (the image's for the stem, x's otherwise)"""
        self.mods, self.x, self.res, self.outs, self.stem = mods, x, res, outs, stem
        c = mods[0].conv
        self.k, self.s, self.p = c.kernel_size[0], c.stride[0], c.padding[0]
        self.Ks = [m.conv.out_channels for m in mods]
        self.K = sum(self.Ks)
        self.C = c.in_channels
        self.hin, self.win = hin, win
        self.M = outs[0].n * outs[0].h * outs[0].w          # output pixels
        self.pack_kind = ops.PACK_STEM if stem else ops.PACK_FWD
        self.stem_hw = (hin, win) if stem else None
        self.has_bn = hasattr(mods[0], 'bn')
        # torchvision-style FrozenBatchNorm2d put in place by Model.freeze (utils_torch.freeze_bn): constant scale / shift in training too
        self.frozen = self.has_bn and type(mods[0].bn).__name__ == 'FrozenBatchNorm2d'
        assert all((hasattr(m, 'bn') and type(m.bn).__name__ == 'FrozenBatchNorm2d') == self.frozen for m in mods)
        self.act = act_code(mods[0].act)


class DetUnit:
    def __init__(self, conv, x, level):
        self.conv, self.x, self.level = conv, x, level
        self.K = conv.out_channels
        self.Kp = (self.K + 7) // 8 * 8
        self.M = x.n * x.h * x.w


class PoolUnit:
    def __init__(self, x, outs):
        self.x, self.outs = x, outs


class UpUnit:
    def __init__(self, x, out):
        self.x, self.out = x, out


class _Scratch:
    """What the shared scratch buffers have to hold, as the per-unit allocators report it: the largest request for each (elements or
    bytes, whichever that buffer is sized in) and the widest ConvUnit."""

    def __init__(self):
        self.stats = self.dy = self.wg = self.bnws = self.f1 = 1
        self.kmax = 0

    def add(self, **sizes):
        for k, n in sizes.items():
            setattr(self, k, max(getattr(self, k), n))


class _BackwardList:
    """The backward launch list while Plan._compile_backward builds it: the records, the side stream weight gradients fork to, and what the
    units of the reversed walk have to know of each other."""

    def __init__(self, plan, side):
        self.plan, self.side = plan, side       # side: ops.SideStream, or None = everything on the main stream
        self.recs, self.nfork = [], 0
        self.nslot, self.slot_user = 0, {}      # dy ring: slots handed out so far; slot -> token of the fork that read it last
        # Producer-side statistics: `last[id(v)]` = the launch record that wrote the LAST contribution of v's gradient (kind, index into
        # recs when it is a launch which can serve statistics, channel offset of v inside that launch's output, slab count); remake[index]
        # rebuilds that record with statistics requests, pending[index] are the requests made of it so far.
        self.last, self.pending, self.remake = {}, {}, {}
        self.grad_log = []                      # (parameter, position of the record that writes its gradient)

    def add(self, rec):
        self.recs.append(rec)

    def grad(self, p):
        """p's view of the flat gradient buffer, for the record appended NEXT (its position is what the bucket marks go by)"""
        self.grad_log.append((p, len(self.recs)))
        return self.plan._grad_views(p)

    def wgrad(self, make, pixels=None, reads_slot=None):
        """A weight-gradient launch, make(workspace): forked to the side stream, or inline on the main stream when there is none or the
        layer has fewer than FORK_MIN_PIXELS output pixels — then on a workspace of its own beside the side stream's split slabs."""
        if SKIP_WGRAD:              # timing experiment only (gradients wrong): what the step costs without the weight-gradient stream
            return
        if self.side is None:
            self.recs.append(make(self.plan.wg_ws))
        elif pixels is not None and pixels < FORK_MIN_PIXELS:
            self.recs.append(make(self.plan.wg_ws_main))
        else:
            self.recs.append(('@fork', self.side, [make(self.plan.wg_ws)], self.nfork))
            if reads_slot is not None:
                self.slot_user[reads_slot] = self.nfork
            self.nfork += 1

    def next_slot(self):
        """the dy ring slot of the next unit; the weight gradient that last read it must be done"""
        slot = self.nslot % len(self.plan.dy_ring)
        self.nslot += 1
        if slot in self.slot_user:
            self.recs.append(('@join', self.side, self.slot_user.pop(slot)))
        return slot

    def note_grad(self, xv, kind, make=None, slabs=0):
        """the record appended last wrote (so far) the last contribution to xv's gradient; make(requests) rebuilds it serving statistics"""
        idx = None if make is None else len(self.recs) - 1
        for pv, off in ([(xv, 0)] if xv.parts is None else xv.parts):
            self.last[id(pv)] = (kind, idx, off, slabs)
        if idx is not None:
            self.remake[idx] = make

    def add_producer(self, xv, kind, make, slabs):
        self.recs.append(make(None))
        self.note_grad(xv, kind, make, slabs)

    def producers(self, outs):
        """`last` of every value of `outs` when each can still serve that value's statistics (a launch takes two requests), else None"""
        prod = [self.last.get(id(o)) for o in outs]
        kinds = ('dgrad', 'fused') if PRODUCER_STATS == '1' else ('fused',)
        ok = all(q is not None and q[0] in kinds and q[3] > 0 and o.gfinal is None and o.c % 8 == 0 and q[2] % 8 == 0 and
                 len(self.pending.get(q[1], [])) < 2 for q, o in zip(prod, outs))
        if ok and len(outs) == 2 and prod[0][1] == prod[1][1]:
            ok = len(self.pending.get(prod[0][1], [])) == 0
        return prod if ok else None


def act_code(act):
    if isinstance(act, nn.SiLU):
        return ops.ACT_SILU
    if isinstance(act, nn.Identity):
        return ops.ACT_NONE
    raise _lib.HdyError(f'activation {type(act).__name__} has no HIP kernel on this path (SiLU / Identity only)')


def _is(m, name):
    return type(m).__name__ == name


class Plan:
    def __init__(self, backbone, neck, head, shape, dtype, training, device, grad_store=None, taps=(), tap_params=(), sync=None):
        """backbone / neck: the metayolo CSPDarkNet / FPN containers (neck, head may be None);
        head: Detect module or None; shape = (B, 3, H, W).
        Feature-input plans (FPN.forward / Detect.forward called on bare feature maps): backbone is None and shape is
        {layer index: (B, C, H, W)}; eval only."""
        self.dtype, self.training, self.device = dtype, training, device
        # SyncBatchNorm (train.py --sync-bn; reference: train.py:281-283): None = per-rank statistics; True = the default process group, or a
        # group object: every training BatchNorm all-reduces its (SUM, SUM2, count) forward and its (SUM du, SUM du*xhat, count) backward
        self.sync = sync if training else None
        self.ext_shapes = dict(shape) if isinstance(shape, dict) else None
        if self.ext_shapes is not None:
            if backbone is not None or training:
                raise _lib.HdyError('feature-input plans are neck/head-only and forward-only')
            self.B, self.Cin, self.H, self.W = next(iter(self.ext_shapes.values()))[0], 0, 0, 0
        else:
            self.B, self.Cin, self.H, self.W = shape
        self.input = None
        self.ext = {}
        self.vals, self.units = [], []
        self.grad_store = grad_store
        # taps: layer indices whose outputs also feed modules outside the plan (hnet's segmentation header on the pyramid): their
        # gradient buffers are pre-filled from outside before the backward list runs; tap_params: those modules' parameters (their
        # gradients are written into the flat store by the outside backward, or zeroed when it did not run)
        self.tap_keys, self.tap_params = list(taps), list(tap_params)
        self.tap_grads_ready = False
        self.bucket_hook = None         # engine: called as hook(a, b, side_stream) when gradient elements [a, b) of the flat buffer are final
        self._order = 0
        self._trace(backbone, neck, head)
        self._allocate()
        self.packs = ops.PackTable(device)          # every weight re-pack of the plan, one launch per step
        self.bn_eval = ops.BnEvalTable(device)      # eval plans: every BatchNorm's folded scale / shift, one launch per forward
        self.fwd = self._compile_forward()
        self.bwd = self._compile_backward() if training else None
        # the two launch lists have fixed pointers and shapes: after one eager run each they are captured into hipGraphs and
        # replayed with one call (the eager lists are ~350 / ~450 launches per step for yolov5s)
        self._graphs = {'fwd': None, 'bwd': None}
        self._runs = {'fwd': 0, 'bwd': 0}
        self._progs = {}                # 'fwd' / 'bwd' -> ops.Program of that list, compiled at its first replay
        self._bn_running = None         # bn_running()'s list, built at its first call
        self._pack_stream = None        # PACK_SIDE: the stream the weight re-pack runs on

    # ------------------------------------------------------------------ tracing
    def _val(self, n, h, w, c, name):
        v = Val(n, h, w, c, name, self._order)
        self._order += 1
        self.vals.append(v)
        return v

    def _use(self, v):
        v.last_use = self._order

    def _conv(self, mods, x, res=None, stem=False):
        c0 = mods[0].conv
        for m in mods:
            c = m.conv
            if c.groups != 1 or c.dilation[0] != 1 or c.kernel_size[0] != c.kernel_size[1] or c.stride[0] != c.stride[1]:
                raise _lib.HdyError('grouped / dilated / non-square convolutions are outside the hot path')
            assert (c.kernel_size, c.stride, c.padding, c.in_channels) == (c0.kernel_size, c0.stride, c0.padding, c0.in_channels)
        k, s, p = c0.kernel_size[0], c0.stride[0], c0.padding[0]
        if stem:
            n, h, w = self.B, self.H, self.W
        else:
            n, h, w = x.n, x.h, x.w
            self._use(x)
        if res is not None:
            self._use(res)
        ho, wo = ops.out_dim(h, k, s, p), ops.out_dim(w, k, s, p)
        outs = [self._val(n, ho, wo, m.conv.out_channels, 'conv') for m in mods]
        u = ConvUnit(mods, x, res, outs, stem, h, w)
        self.units.append(u)
        if res is not None and self.training:
            if res.cat is not None or res.parts is not None:
                raise _lib.HdyError('shortcut from a concat member is not plannable')
            res.galias = outs[0]
        return outs

    def _concat(self, vals):
        n, h, w = vals[0].n, vals[0].h, vals[0].w
        cat = self._val(n, h, w, sum(v.c for v in vals), 'cat')
        off, cat.parts = 0, []
        for v in vals:
            if v.cat is not None or v.parts is not None:
                raise _lib.HdyError('a tensor may sit in one concat only (nested / shared concats are not planned)')
            assert (v.n, v.h, v.w) == (n, h, w)
            v.cat, v.off = cat, off
            cat.parts.append((v, off))
            off += v.c
            self._use(v)
        return cat

    def _module(self, m, x):
        t = type(m).__name__
        if t == 'Conv':
            return self._conv([m], x, stem=(x is None))[0]
        if t == 'Bottleneck':
            h = self._conv([m.cv1], x)[0]
            return self._conv([m.cv2], h, res=x if m.add else None)[0]
        if t == 'C3':
            fuse = (self.training and hasattr(m.cv1, 'bn') and hasattr(m.cv2, 'bn') and type(m.cv1.bn) is type(m.cv2.bn)
                    and m.cv1.conv.weight.requires_grad == m.cv2.conv.weight.requires_grad)
            if fuse:
                a, b = self._conv([m.cv1, m.cv2], x)
            else:
                a, b = self._conv([m.cv1], x)[0], self._conv([m.cv2], x)[0]
            for bt in m.m:
                a = self._module(bt, a)
            return self._conv([m.cv3], self._concat([a, b]))[0]
        if t == 'SPPF':
            if m.m.kernel_size != 5:
                raise _lib.HdyError('SPPF pooling kernel must be 5')
            a = self._conv([m.cv1], x)[0]
            self._use(a)
            ys = [self._val(a.n, a.h, a.w, a.c, 'pool') for _ in range(3)]
            self.units.append(PoolUnit(a, ys))
            return self._conv([m.cv2], self._concat([a] + ys))[0]
        if t == 'Upsample':
            if m.mode != 'nearest' or float(m.scale_factor) != 2.0:
                raise _lib.HdyError('only 2x nearest upsampling is on the hot path')
            self._use(x)
            out = self._val(x.n, 2 * x.h, 2 * x.w, x.c, 'up')
            self.units.append(UpUnit(x, out))
            return out
        if t == 'Concat':
            if m.d != 1:
                raise _lib.HdyError('Concat along a dimension other than channels')
            return self._concat(x)
        if t == 'Sequential':
            for sub in m:
                x = self._module(sub, x)
            return x
        raise _lib.HdyError(f'module {t} is outside the metayolo hot path (no HIP plan for it)')

    def _trace(self, backbone, neck, head):
        outs = {}
        if backbone is None:
            for k, (b, c, h, w) in self.ext_shapes.items():
                if c % 8:
                    raise _lib.HdyError(f'feature map {k} has {c} channels: HIP plans take multiples of 8')
                outs[k] = self._val(b, h, w, c, 'input')
                outs[k].index = k
            self.ext = dict(outs)
            backbone = []
        first = backbone[0] if len(backbone) else None
        is_stem = (type(first).__name__ == 'Conv' and self.Cin == 3 and first.conv.kernel_size == (6, 6)
                   and first.conv.stride == (2, 2) and first.conv.padding == (2, 2))
        if is_stem:
            x = None                       # the 6x6/s2 stem reads the padded 4-channel image directly
        elif self.ext:
            x = None
        else:
            if self.Cin % 8:
                raise _lib.HdyError(f'input with {self.Cin} channels: only the 6x6/s2 RGB stem or channel counts that are '
                                    'multiples of 8 can enter a HIP plan')
            x = self.input = self._val(self.B, self.H, self.W, self.Cin, 'input')
        for i, m in enumerate(backbone):
            x = self._module(m, x)
            x.index = i
            outs[i] = x
        self.feature_keys = list(getattr(backbone, 'save', [len(backbone) - 1])) if len(backbone) else list(self.ext)
        if neck is not None:
            cur = None
            for m in neck:
                f = m.f
                if isinstance(f, int):
                    src = cur if f == -1 else outs[f]
                else:
                    src = [cur if j == -1 else outs[j] for j in f]
                cur = self._module(m, src)
                cur.index = m.i
                outs[m.i] = cur
            self.feature_keys = list(neck.save)
        self.outs = outs
        # one or several Detect headers on the same feature maps (yolo.py:62-81 loops over self.headers): their 1x1 detection convs are
        # all units of this plan; det_views() lists the logits header after header, level after level
        heads = [] if head is None else (list(head) if isinstance(head, (list, tuple)) else [head])
        self.det_units, self.det_split = [], []
        for hi, hd in enumerate(heads):
            f = hd.f if isinstance(hd.f, (list, tuple)) else [hd.f]
            for l, (j, conv) in enumerate(zip(f, hd.m)):
                self._use(outs[j])
                u = DetUnit(conv, outs[j], l)
                u.head, u.na, u.no = hi, hd.na, hd.no
                self.units.append(u)
                self.det_units.append(u)
            self.det_split.append(len(f))
        if heads:
            self.na, self.no = heads[0].na, heads[0].no
        if len(heads) > 1 and any(getattr(hd, 'seg', None) is not None for hd in heads):
            raise _lib.HdyError('a mask branch is supported on single-header models only')
        head = heads[0] if len(heads) == 1 else None       # the mask branch below belongs to a lone header
        # mask branch: one 3x3 Conv per level, top-down module order (yolo_head.py:123-124, :170-173); their outputs
        # feed roi_align outside the plan and their output gradients arrive from there (MaskBranch in engine.py)
        self.mask_vals = []
        if head is not None and getattr(head, 'seg', None) is not None:
            f = head.f if isinstance(head.f, (list, tuple)) else [head.f]
            vals = [self._module(m, outs[f[-i]]) for i, m in enumerate(head.seg, 1)]
            self.mask_vals = vals[::-1]
        self.mask_grads_ready = False
        self.seg_h_params = list(head.seg_h.parameters()) if self.mask_vals else []

    def _fusable_1x1(self, u):
        """Backward of this unit as ONE launch after the statistics pass (hdy_conv1x1_bwd_fused): 1x1 / stride 1 Conv + live BatchNorm +
        SiLU in bf16 with a kernel instance for its widths."""
        return (FUSED_1X1 and not USE_GRAPHS and self.training and self.dtype == torch.bfloat16 and not u.stem and u.k == 1 and u.s == 1
                and u.p == 0 and u.has_bn and not u.frozen and u.act == ops.ACT_SILU and ops.fused_1x1_ok(u.C, u.K, self.dtype)
                and all(m.conv.out_channels % 8 == 0 for m in u.mods))

    # ------------------------------------------------------------------ memory
    def _new(self, *shape, dtype=None, zero=False):
        f = torch.zeros if zero else torch.empty
        return f(shape, dtype=dtype or self.dtype, device=self.device)

    def _allocate(self):
        self._alloc_activations()
        need = _Scratch()
        alloc = {ConvUnit: self._alloc_conv, DetUnit: self._alloc_det, PoolUnit: self._alloc_pool}
        for u in self.units:
            if type(u) in alloc:
                alloc[type(u)](u, need)
        if self.training:
            self._alloc_det_grads()
            self._alloc_scratch(need)
            self._alloc_gradients()

    def _alloc_activations(self):
        for v in self.vals:
            if v.parts is not None or v.cat is None:
                v.buf = self._new(v.n, v.h, v.w, v.c)
        for v in self.vals:
            if v.cat is not None:
                v.buf = v.cat.buf
        self.prep = self._new(self.B, self.H + 4, self.W + 4, 4)

    def _alloc_conv(self, u, need):
        dt, f32, o = self.dtype, torch.float32, u.outs[0]
        u.wp = ops.pack_alloc(u.K, u.C, u.k, u.k, u.s, u.p, u.pack_kind, dt, self.device)
        u.scale, u.shift = self._new(u.K, dtype=f32), self._new(u.K, dtype=f32)
        if not self.training:
            return
        if not u.has_bn:
            raise _lib.HdyError('training a fused (BN-folded) model is not supported: build the model unfused')
        u.yraw = self._new(o.n, o.h, o.w, u.K)
        if u.frozen:
            u.mean = u.invstd = None
            u.mtiles = 0
        else:
            u.mean, u.invstd = self._new(u.K, dtype=f32), self._new(u.K, dtype=f32)
            u.mtiles = ops.stat_slabs(o.n, u.hin, u.win, u.C, u.K, u.k, u.k, u.s, u.p, dt)
        need.add(stats=u.mtiles * 2 * u.K, dy=u.M * u.K, bnws=ops.bn_bwd_ws_floats(u.M, u.K), kmax=u.K,
                 wg=ops.wgrad_ws_bytes(o.n, u.hin, u.win, u.C, u.K, u.k, u.k, u.s, u.p, dt, stem=u.stem))
        if self._fusable_1x1(u):
            need.add(f1=ops.fused_1x1_ws_bytes(u.M, u.C, u.K))
        if not u.stem:
            u.wpd = ops.pack_alloc(u.K, u.C, u.k, u.k, u.s, u.p, ops.PACK_DGRAD, dt, self.device)

    def _alloc_det(self, u, need):
        x, dt = u.x, self.dtype
        u.wp = ops.pack_alloc(u.K, x.c, 1, 1, 1, 0, ops.PACK_FWD, dt, self.device)
        u.logits = self._new(x.n, x.h, x.w, u.Kp, dtype=torch.float32, zero=True)
        if self.training:
            u.wpd = ops.pack_alloc(u.Kp, x.c, 1, 1, 1, 0, ops.PACK_DGRAD, dt, self.device)
            need.add(wg=ops.wgrad_ws_bytes(x.n, x.h, x.w, x.c, u.Kp, 1, 1, 1, 0, dt), bnws=ops.bn_bwd_ws_floats(u.M, u.Kp))

    def _alloc_pool(self, u, need):
        if self.training:
            a = u.x
            u.idx = [self._new(a.n, a.h, a.w, a.c, dtype=torch.uint8) for _ in range(3)]

    def _alloc_det_grads(self):
        # logits gradients of all levels live in one flat buffer (one scale launch, one owner)
        sizes = [u.M * u.Kp for u in self.det_units]
        self.gdet_flat = self._new(max(sum(sizes), 1), zero=True)
        off = 0
        for u, n in zip(self.det_units, sizes):
            u.gdet = self.gdet_flat[off:off + n].view(u.x.n, u.x.h, u.x.w, u.Kp)
            off += n
        self.loss_out = self._new(4, dtype=torch.float32, zero=True)
        self.loss_call = None

    def _alloc_scratch(self, need):
        f32 = torch.float32
        self.stats = self._new(need.stats, dtype=f32)
        # BN-backward output of the layer in flight; a small ring, so that the weight-gradient kernels of the previous layers
        # (side stream) may still be reading theirs while the main stream moves on
        self.dy_ring = [self._new(need.dy) for _ in range(DY_RING if SIDE_WGRAD else 1)]
        self.wg_ws = self._new(need.wg // 4 + 16, dtype=f32)
        self.wg_ws_main = self._new(need.wg // 4 + 16, dtype=f32) if (FORK_MIN_PIXELS > 0 and SIDE_WGRAD) else self.wg_ws
        self.bn_c12 = self._new(2, need.kmax, dtype=f32)     # c1 / c2 of the unit in flight
        self.f1_ws = self._new(need.f1 // 4 + 16, dtype=f32)      # weight-gradient slabs of the fused 1x1 backward (main stream: not shared with wg_ws)
        self.bn_ws = self._new(need.bnws, dtype=f32)
        self.fin_ws = self._new(32 * 2 * need.kmax, dtype=torch.float64)
        self.sync_sums = self._new(2 * need.kmax + 1, dtype=torch.float64) if self.sync else None

    def _alloc_gradients(self):
        # gradient storage mirrors activation storage
        for v in reversed(self.vals):
            if v.cat is None and (v.galias is None or v.parts is not None):
                v.gbuf = self._new(v.n, v.h, v.w, v.c)
        for v in self.vals:
            if v.cat is not None:
                v.gbuf, v.goff = v.cat.gbuf, v.off
        for v in reversed(self.vals):      # shortcut inputs share the gradient storage of the block output
            if v.galias is not None and v.cat is None:
                o = v.galias
                v.gbuf, v.goff = o.gbuf, o.goff
        for u in self.units:
            if isinstance(u, PoolUnit):
                u.x.gfinal = self._new(u.x.n, u.x.h, u.x.w, u.x.c)

    # ------------------------------------------------------------------ parameter access
    def _bn(self, m):
        return m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var

    def _grad_views(self, p):
        return self.grad_store.view_of(p)

    # ------------------------------------------------------------------ forward
    def _compile_forward(self):
        emit = {ConvUnit: self._fwd_conv, PoolUnit: self._fwd_pool, UpUnit: self._fwd_up, DetUnit: self._fwd_det}
        recs = []
        for u in self.units:
            emit[type(u)](recs, u)
        return recs

    def _fwd_pool(self, recs, u):
        recs.append(ops.rec_sppf_pool_fwd(u.x.t(), u.outs[0].t(), u.outs[1].t(), u.outs[2].t(), u.idx if self.training else None))

    def _fwd_up(self, recs, u):
        recs.append(ops.rec_upsample_fwd(u.x.t(), u.out.t()))

    def _fwd_det(self, recs, u):
        self.packs.add(u.conv.weight, None, 1, 0, ops.PACK_FWD, u.wp)
        recs.append(ops.rec_conv_fwd(u.x.t(), u.wp, u.logits[..., :u.K], u.K, 1, 1, 1, 0, shift=u.conv.bias))

    def _fwd_conv(self, recs, u):
        (self._fwd_conv_train if self.training else self._fwd_conv_eval)(recs, u, self.prep if u.stem else u.x.t())

    def _fwd_conv_eval(self, recs, u, x):
        """one launch: BatchNorm folded into the epilogue's scale / shift through the bn_eval table, or (a BN-folded model) the bias alone"""
        m, o = u.mods[0], u.outs[0]
        self.packs.add(m.conv.weight, None, u.s, u.p, u.pack_kind, u.wp)
        if u.has_bn:
            self.bn_eval.add(*self._bn(m), u.scale, u.shift, eps=m.bn.eps)
            scale, shift = u.scale, u.shift
        else:
            scale, shift = None, m.conv.bias
        res = u.res.t() if u.res is not None else None
        recs.append(ops.rec_conv_fwd(x, u.wp, o.t(), u.K, u.k, u.k, u.s, u.p, scale=scale, shift=shift, act=u.act, stem_hw=u.stem_hw, res=res))

    def _fwd_conv_train(self, recs, u, x):
        """the raw convolution, leaving per-tile statistics slabs unless the BatchNorm is frozen, then the BatchNorm forward of _bn_fwd_mode(u)"""
        wb = u.mods[1].conv.weight if len(u.mods) > 1 else None
        self.packs.add(u.mods[0].conv.weight, wb, u.s, u.p, u.pack_kind, u.wp)
        stats = None if u.frozen else self.stats[:u.mtiles * 2 * u.K].view(u.mtiles, 2, u.K)
        recs.append(ops.rec_conv_fwd(x, u.wp, u.yraw, u.K, u.k, u.k, u.s, u.p, stats=stats, stem_hw=u.stem_hw))
        getattr(self, '_bn_fwd_' + self._bn_fwd_mode(u))(recs, u, stats)

    def _bn_fwd_mode(self, u):
        """How a training ConvUnit's scale / shift come about: 'sync' (slabs -> fp64 sums -> all-reduce -> one finalize per module), 'pair' (the
        C3 pair: one finalize over the whole 2c-wide raw tensor), 'single' (one finalize per module), 'frozen' (constant coefficients from the
        running statistics, no slabs)."""
        if self.sync and not u.frozen:
            return 'sync'
        if self._pair_apply(u):
            return 'pair'
        return 'frozen' if u.frozen else 'single'

    @staticmethod
    def _pair_apply(u):
        """two live modules share the raw tensor and nothing is added: both halves are normalised in one pass"""
        return len(u.mods) == 2 and not u.frozen and u.res is None

    def _bn_fwd_apply(self, recs, u, coeffs=None):
        """The normalise + activation (+ residual) pass behind the coefficient records coeffs(m, k0, K) of the modules: one pass over both halves
        behind both records for a pair, else every module's record followed by its own pass."""
        pair = self._pair_apply(u)
        res = u.res.t() if u.res is not None else None
        for m, o, ch in self._channels(u):
            if coeffs is not None:
                recs.append(coeffs(m, ch.start, ch.stop - ch.start))
            if not pair:
                recs.append(ops.rec_bn_act_fwd(u.yraw[..., ch], u.scale[ch], u.shift[ch], o.t(), res=res, act=u.act))
        if pair:
            recs.append(ops.rec_bn_act_fwd_pair(u.yraw, u.scale, u.shift, u.outs[0].t(), u.outs[1].t(), act=u.act))

    # One emitter per mode.  The per-module coefficient records take open-ended slices [k0:] of the unit's K-wide vectors (the kernels write K
    # of them from there on).
    def _bn_fwd_sync(self, recs, u, stats):
        buf = self.sync_sums[:2 * u.K + 1]              # [SUM | SUM2 | count]
        recs.append(ops.rec_bn_slab_sums(stats, u.mtiles, u.K, u.M, buf))
        recs.append(self._sync_call(buf))
        self._bn_fwd_apply(recs, u, lambda m, k0, K: ops.rec_bn_finalize_sums(
            buf, u.K, k0, K, K, self._bn(m), None, u.scale[k0:], u.shift[k0:], u.mean[k0:], u.invstd[k0:], eps=m.bn.eps, momentum=m.bn.momentum))

    def _bn_fwd_pair(self, recs, u, stats):
        ma, mb = u.mods
        assert ma.bn.eps == mb.bn.eps and ma.bn.momentum == mb.bn.momentum
        recs.append(ops.rec_bn_finalize_pair(stats, u.mtiles, u.K, ma.conv.out_channels, u.M, self._bn(ma), self._bn(mb), u.scale, u.shift,
                                             u.mean, u.invstd, eps=ma.bn.eps, momentum=ma.bn.momentum, ws=self.fin_ws))
        self._bn_fwd_apply(recs, u)

    def _bn_fwd_single(self, recs, u, stats):
        self._bn_fwd_apply(recs, u, lambda m, k0, K: ops.rec_bn_finalize(
            stats[:, :, k0:], u.mtiles, K, u.M, *self._bn(m), u.scale[k0:], u.shift[k0:], u.mean[k0:], u.invstd[k0:], stats_ld=u.K, ws=self.fin_ws))

    def _bn_fwd_frozen(self, recs, u, stats):
        self._bn_fwd_apply(recs, u, lambda m, k0, K: ops.rec_bn_eval_coeffs(*self._bn(m), u.scale[k0:k0 + K], u.shift[k0:k0 + K], eps=m.bn.eps))

    def _replay(self, key, recs):
        if not USE_GRAPHS:
            if not ops.USE_EXEC:
                return ops.run(recs)
            # the list is static: compiled once into words for hdy_exec_run (one C call per stretch between host callbacks) and replayed
            prog = self._progs.get(key)
            if prog is None or prog.records is not recs or prog.nrec != len(recs):
                prog = self._progs[key] = ops.Program(recs)
            return prog.run()
        g = self._graphs[key]
        if g is None:
            self._runs[key] += 1
            if self._runs[key] < 2:
                return ops.run(recs)                 # first call eager: lazy one-time host setup happens here
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                ops.run(recs)
            self._graphs[key] = g
        g.replay()

    def bn_counters(self):
        return [m.bn.num_batches_tracked for u in self.units if isinstance(u, ConvUnit) and u.has_bn and not u.frozen for m in u.mods]

    def bn_running(self):
        """running_mean / running_var of every live BatchNorm: the training forward writes them through raw pointers"""
        if self._bn_running is None:
            self._bn_running = [t for u in self.units if isinstance(u, ConvUnit) and u.has_bn and not u.frozen for m in u.mods
                                for t in (m.bn.running_mean, m.bn.running_var)]
        return self._bn_running

    def run_forward_features(self, feats):
        """Feature-input plan: feats {layer index: NCHW tensor} -> det logits views (empty without a head)."""
        for k, v in self.ext.items():
            f = feats[k]
            ops.require_gpu(f)
            assert tuple(f.shape) == (v.n, v.c, v.h, v.w), (k, tuple(f.shape), (v.n, v.c, v.h, v.w))
            ops.run([ops.rec_nchw_to_nhwc(f.float().contiguous(), v.t())])
        self.packs.run(skip_unchanged=not self.training)
        self.bn_eval.run(skip_unchanged=not self.training)
        self._replay('fwd', self.fwd)
        return self.det_views()

    def run_forward(self, images):
        ops.require_gpu(images)
        if images.dtype != torch.float32 or not images.is_contiguous():
            images = images.float().contiguous()
        assert tuple(images.shape) == (self.B, self.Cin, self.H, self.W), (images.shape, self.B, self.H, self.W)
        assert images.shape[1] == self.Cin
        return self._run_forward(ops.rec_stem_prep(images, self.prep) if self.input is None else ops.rec_nchw_to_nhwc(images, self.input.t()))

    def run_forward_tiles(self, slide, origins, first, count):
        """run_forward with the batch taken from an 8-bit slide on the device: tiles [first, first + count) of the origin table (int32 [n][2]
        device tensor of (x0, y0)) are gathered straight into the buffer the first convolution reads (hdy_slide_tiles_u8) — no float slide,
        no NCHW batch, no stem_prep pass."""
        if count != self.B or self.Cin != 3:
            raise _lib.HdyError(f'run_forward_tiles: {count} tiles of 3 channels for a plan of batch {self.B} with {self.Cin} input channels')
        if self.input is None:
            return self._run_forward(ops.rec_slide_tiles(slide, origins, first, count, self.prep))
        return self._run_forward(ops.rec_slide_tiles(slide, origins, first, count, self.input.t(), pad=0))

    def _run_forward(self, input_rec):
        """the forward list behind the record that fills the first convolution's input buffer"""
        pack_side = self.training and PACK_SIDE
        if pack_side:
            # the per-step weight re-pack (one launch, ~50 us of gathers at yolov5s) depends on the optimizer's update, not on the images: it runs on a
            # second stream beside the input conversion (an HBM stream of ~90 us) and joins in front of the first convolution
            main = torch.cuda.current_stream(self.device)
            if self._pack_stream is None:
                self._pack_stream = torch.cuda.Stream(device=self.device)
            self._pack_stream.wait_stream(main)
            with torch.cuda.stream(self._pack_stream):
                self.packs.run(skip_unchanged=False)
        ops.run([input_rec])
        if pack_side:
            main.wait_stream(self._pack_stream)
        else:
            self.packs.run(skip_unchanged=not self.training)
        self.bn_eval.run(skip_unchanged=not self.training)
        self._replay('fwd', self.fwd)
        if self.training:
            torch._foreach_add_(self.bn_counters(), 1)
            # the kernels updated the running statistics in place: move their version counters as torch's own BatchNorm would, so that
            # `_version`-keyed caches (ops.BnEvalTable of an eval plan on the same live model) see the change
            torch._C._increment_version(self.bn_running())
        return self.det_views()

    def det_views(self):
        views = []
        for u in self.det_units:
            x = u.x
            views.append(u.logits[..., :u.K].view(x.n, x.h, x.w, u.na, u.no).permute(0, 3, 1, 2, 4))
        return views

    def mask_features(self):
        """NHWC views of the mask branch's per-level feature maps (level order)."""
        return [v.t() for v in self.mask_vals]

    def feature(self, index):
        """NCHW-shaped (channels-last strided) view of layer `index`'s output."""
        return self.outs[index].t().permute(0, 3, 1, 2)

    # ------------------------------------------------------------------ backward
    def _contrib(self, v):
        """Is a gradient contribution to v an accumulation?  Marks the storage initialised."""
        if v.cat is not None:
            if v.cat.ginit or v.ginit:
                return True
            v.ginit = True
            return False
        if v.galias is not None:
            return True            # storage already holds the block output's gradient (shortcut identity)
        acc = v.ginit
        v.ginit = True
        return acc

    def _sync_call(self, buf):
        """launch-list record that all-reduces a SyncBatchNorm sums buffer in place (on the current stream, as every other record)"""
        import torch.distributed as dist
        group = None if self.sync is True else self.sync
        return ('@call', lambda buf=buf, group=group: dist.all_reduce(buf, group=group))

    def _mark_needs_grad(self):
        """Model.freeze: a tensor needs a gradient only if something trainable lies upstream of it.  Sets `needs_grad` of every unit output
        and of every concat a unit reads; the backward walk reads that and nothing else: units without trainable parameters below frozen
        inputs are skipped altogether, frozen filters skip their weight gradient."""
        def trainable(u):
            ps = [m.conv.weight for m in u.mods]
            if u.has_bn and not u.frozen:
                ps += [q for m in u.mods for q in (m.bn.weight, m.bn.bias)]
            return any(q.requires_grad for q in ps)

        def up(v):                                   # needs_grad of a (possibly concatenated) input value; None: the stem's image, no shortcut
            if v is not None and v.parts is not None:
                v.needs_grad = any(pv.needs_grad for pv, _ in v.parts)
            return v is not None and v.needs_grad

        for v in list(self.ext.values()) + ([self.input] if self.input is not None else []):
            v.needs_grad = False
        for k in self.tap_keys:
            v = self.outs[k]
            if v.cat is not None or v.parts is not None or v.galias is not None:
                raise _lib.HdyError(f'layer {k} cannot be tapped: its gradient storage is shared (concat member / shortcut)')
        for u in self.units:
            below = up(u.x)
            if isinstance(u, ConvUnit):
                below = up(u.res) or below or trainable(u)
            for o in ([] if isinstance(u, DetUnit) else [u.out] if isinstance(u, UpUnit) else u.outs):
                o.needs_grad = below

    def _compile_backward(self):
        self._mark_needs_grad()
        for v in self.vals:
            v.ginit = False
        for k in self.tap_keys:
            self.outs[k].ginit = True       # holds the outside consumer's gradient when the list starts: everything else accumulates
        # Weight gradients are consumed only by the optimizer: with SIDE_WGRAD they run on a second stream beside the
        # dgrad / BN-backward chain (which is what the next layer waits for), filling the CUs that the many small launches
        # of the 20x20 and 40x40 layers leave idle.
        b = _BackwardList(self, ops.SideStream(self.device) if SIDE_WGRAD else None)
        emit = {DetUnit: self._bwd_det, UpUnit: self._bwd_up, PoolUnit: self._bwd_pool, ConvUnit: self._bwd_conv}
        for u in reversed(self.units):
            emit[type(u)](b, u)
        recs, side = b.recs, b.side
        for idx, reqs in b.pending.items():                 # rebuild the producers with the statistics requests they serve
            recs[idx] = b.remake[idx](reqs)
        self.producer_stat_units = sum(len(v) for v in b.pending.values())
        self._mark_buckets(recs, side, b.grad_log)
        last_fork = next((r[3] for r in reversed(recs) if r[0] == '@fork'), None)      # in LIST order (tokens need not follow it)
        if side is not None and last_fork is not None:
            recs.append(('@join', side, last_fork))             # side-stream work is in order: the last fork covers all
        return recs

    def _bwd_det(self, b, u):
        x = u.x
        tmp = self._det_bias_tmp(u)
        b.add(ops.rec_colsum(u.gdet, tmp, self.bn_ws))
        b.add(ops.rec_copy_f32(tmp[:u.K], b.grad(u.conv.bias)))                                # Kp-padded column sums -> the bias gradient
        gw = b.grad(u.conv.weight)
        b.wgrad(lambda ws: ops.rec_conv_wgrad(x.t(), u.gdet, gw, None, 1, 1, 1, 0, ws), pixels=u.M)
        if not x.needs_grad:
            return
        self.packs.add(u.conv.weight, None, 1, 0, ops.PACK_DGRAD, u.wpd, K=u.Kp)
        acc = self._contrib(x)
        b.add_producer(x, 'dgrad', lambda st: ops.rec_conv_dgrad(u.gdet, u.wpd, x.g(), 1, 1, 1, 0, accumulate=acc, stats=st),
                       self._dgrad_slabs(x, u.Kp, 1, 1, 0))

    def _bwd_up(self, b, u):
        if u.x.needs_grad:
            b.add(ops.rec_upsample_bwd(u.out.gread(), u.x.g(), accumulate=self._contrib(u.x)))
            b.note_grad(u.x, 'other')

    def _bwd_pool(self, b, u):
        a = u.x
        if a.needs_grad:
            b.add(ops.rec_sppf_pool_bwd(a.g(), u.outs[0].g(), u.outs[1].g(), u.outs[2].g(), u.idx, a.gfinal))
            b.note_grad(a, 'other')

    def _dgrad_slabs(self, xv, K, k, s, p):
        """statistics slabs a data-gradient launch into xv could serve (0: none)"""
        return ops.conv_dgrad_stat_slabs(xv.n, xv.h, xv.w, xv.c, K, k, k, s, p, self.dtype) if self.dtype == torch.bfloat16 else 0

    def _bn_bwd_mode(self, u, b):
        """How a ConvUnit's BatchNorm / SiLU backward is done: (consumer, statistics mode).
        consumer    who applies it: 'dy' (an apply pass writes a dy tensor for the weight- and data-gradient launches), 'fused_1x1' (the one-launch
                    1x1 backward) or 'fused_stem' (the stem's weight gradient; the stem has no data gradient, so its dy would have that one reader)
        mode        where SUM du, SUM du*xhat come from: 'sync' (local pass + all-reduce), 'producer' (the launches that completed dz), 'pair' (one
                    pass over both halves of a C3 pair), 'single' (one pass per module), 'frozen' (constant scale / shift: no statistics)"""
        live = u.has_bn and not u.frozen
        sync = bool(self.sync) and live
        if self._fusable_1x1(u) and not sync:
            consumer = 'fused_1x1'
        elif (STEM_FUSED and u.stem and live and not sync and len(u.mods) == 1 and u.mods[0].conv.weight.requires_grad
              # the last unit of the backward list only: the c1 / c2 it reads from the statistics workspace on the side stream are not
              # overwritten before the list's final join
              and u is next(q for q in self.units if isinstance(q, ConvUnit))
              and ops.wgrad_stem_fused_ok(self.B, self.H, self.W, u.K, self.dtype)):
            consumer = 'fused_stem'
        else:
            consumer = 'dy'
        if sync:
            mode = 'sync'
        elif (consumer != 'fused_stem' and PRODUCER_STATS != '0' and self.dtype == torch.bfloat16 and live and not USE_GRAPHS
              and b.producers(u.outs) is not None):
            mode = 'producer'
        elif u.frozen:
            mode = 'frozen'
        else:
            mode = 'pair' if len(u.mods) == 2 else 'single'
        return consumer, mode

    @staticmethod
    def _channels(u):
        """(module, output value, its channel slice of the unit's K-wide tensors) of every module of a ConvUnit"""
        k0 = 0
        for m, o in zip(u.mods, u.outs):
            yield m, o, slice(k0, k0 + m.conv.out_channels)
            k0 += m.conv.out_channels

    # One emitter per statistics mode.  dy: the tensor to write, None when a fused consumer applies the coefficients itself; each returns the
    # (c1, c2) that consumer reads.
    def _bn_bwd_sync(self, b, u, dy, M):
        # SyncBatchNorm: local statistics pass (local dgamma / dbeta: the gradient all-reduce sums them), its partial slabs -> fp64 sums
        # -> all-reduce -> c1 / c2 of the GLOBAL batch in the bn_c12 rows -> one apply pass
        c1, c2 = self.bn_c12[0, :u.K], self.bn_c12[1, :u.K]
        nb = ops.bn_bwd_blocks(M)
        for m, o, ch in self._channels(u):
            K = ch.stop - ch.start
            buf = self.sync_sums[:2 * K + 1]
            b.add(ops.rec_bn_act_bwd(o.gread(), u.yraw[..., ch], u.scale[ch], u.shift[ch], u.mean[ch], u.invstd[ch], None,
                                     b.grad(m.bn.weight), b.grad(m.bn.bias), self.bn_ws, act=u.act))
            b.add(ops.rec_bn_slab_sums(self.bn_ws[:nb * 2 * K].view(nb, 2, K), nb, K, M, buf))
            b.add(self._sync_call(buf))
            b.add(ops.rec_bn_bwd_coeffs_sums(buf, K, c1[ch], c2[ch]))
        self._bn_bwd_apply(b, u, c1, c2, dy)
        return c1, c2

    def _bn_bwd_producer(self, b, u, dy, M):
        # the launches that wrote the last contribution to each output's gradient leave (SUM du, SUM du*xhat) slabs; a finalize launch per
        # module turns them into dgamma / dbeta and c1 / c2 in the bn_c12 rows
        c1, c2 = self.bn_c12[0, :u.K], self.bn_c12[1, :u.K]
        for (m, o, ch), (kind, idx, off, nslabs) in zip(self._channels(u), b.producers(u.outs)):
            slabs = self._new(nslabs, 2, o.c, dtype=torch.float32, zero=True)     # (every workgroup writes its slab, those without tiles zeros)
            b.pending.setdefault(idx, []).append(ops.StatRequest(u.yraw[..., ch], u.scale[ch], u.shift[ch], slabs, off, u.act))
            b.add(ops.rec_bn_bwd_finalize_slabs(slabs, M, u.mean[ch], u.invstd[ch], b.grad(m.bn.weight), b.grad(m.bn.bias), c1[ch], c2[ch]))
        if dy is not None:
            self._bn_bwd_apply(b, u, c1, c2, dy)
        return c1, c2

    def _bn_bwd_pair(self, b, u, dy, M):
        # c1 / c2: where the kernel's finalize stage leaves them in the statistics workspace
        ma, mb = u.mods
        b.add(ops.rec_bn_act_bwd_pair(u.outs[0].gread(), u.outs[1].gread(), u.yraw, u.scale, u.shift, u.mean, u.invstd, dy,
                                      b.grad(ma.bn.weight), b.grad(ma.bn.bias), b.grad(mb.bn.weight), b.grad(mb.bn.bias), self.bn_ws, act=u.act))
        return ops.bn_bwd_coeffs(self.bn_ws, M, u.K)

    def _bn_bwd_single(self, b, u, dy, M):
        # c1 / c2: as for the pair
        for m, o, ch in self._channels(u):
            b.add(ops.rec_bn_act_bwd(o.gread(), u.yraw[..., ch], u.scale[ch], u.shift[ch], u.mean[ch], u.invstd[ch], None if dy is None else dy[..., ch],
                                     b.grad(m.bn.weight), b.grad(m.bn.bias), self.bn_ws, act=u.act))
        return ops.bn_bwd_coeffs(self.bn_ws, M, u.K)

    def _bn_bwd_frozen(self, b, u, dy, M):
        # no statistics, no parameter gradients, no c1 / c2 (and no fused consumer)
        for m, o, ch in self._channels(u):
            b.add(ops.rec_bn_act_bwd(o.gread(), u.yraw[..., ch], u.scale[ch], u.shift[ch], None, None, dy[..., ch], None, None, self.bn_ws, act=u.act))
        return None, None

    def _bn_bwd_apply(self, b, u, c1, c2, dy):
        b.add(ops.rec_bn_act_bwd_apply(u.outs[0].gread(), u.outs[1].gread() if len(u.outs) > 1 else None, u.yraw, u.scale, u.shift, u.mean, u.invstd,
                                       c1, c2, dy, act=u.act))

    def _bwd_conv(self, b, u):
        if not u.outs[0].needs_grad:
            return
        o0, M = u.outs[0], u.M
        consumer, mode = self._bn_bwd_mode(u, b)
        dy = slot = None
        if consumer == 'dy':
            slot = b.next_slot()
            dy = self.dy_ring[slot][:M * u.K].view(o0.n, o0.h, o0.w, u.K)
        c1, c2 = getattr(self, '_bn_bwd_' + mode)(b, u, dy, M)
        x = self.prep if u.stem else u.x.t()
        want_w = any(m.conv.weight.requires_grad for m in u.mods)
        want_x = not u.stem and u.x is not self.input and u.x.needs_grad
        acc, xv = False, u.x
        if want_x:
            wb = u.mods[1].conv.weight if len(u.mods) > 1 else None
            self.packs.add(u.mods[0].conv.weight, wb, u.s, u.p, ops.PACK_DGRAD, u.wpd)
            if xv.parts is not None:
                # writing the whole concat gradient: no part may already hold a partial contribution
                if any(pv.ginit for pv, _ in xv.parts) and not xv.ginit:
                    raise _lib.HdyError('gradient ordering not plannable: a concat input receives gradient before the concat')
                acc = xv.ginit
                xv.ginit = True
            else:
                acc = self._contrib(xv)
        if consumer == 'fused_1x1':
            if want_w or want_x:
                ga = b.grad(u.mods[0].conv.weight) if want_w else None
                gb = b.grad(u.mods[1].conv.weight) if want_w and len(u.mods) > 1 else None
                mk = (lambda st: ops.rec_conv1x1_bwd_fused(
                    u.outs[0].gread(), u.outs[1].gread() if len(u.mods) > 1 else None, u.yraw, u.scale, u.shift, u.mean, u.invstd, c1, c2, x,
                    u.wpd if want_x else None, xv.g() if want_x else None, ga, gb, self.f1_ws, accumulate_dx=acc, stats=st))
                if want_x:
                    b.add_producer(xv, 'fused', mk, ops.fused_1x1_stat_slabs(M, u.C, u.K, self.dtype))
                else:
                    b.add(mk(None))
            return
        ga = b.grad(u.mods[0].conv.weight)          # (logged for frozen filters too: the record behind them bounds their range's mark)
        gb = b.grad(u.mods[1].conv.weight) if len(u.mods) > 1 else None
        if consumer == 'fused_stem':
            b.wgrad(lambda ws: ops.rec_conv_wgrad_stem_fused(x, o0.gread(), u.yraw, u.scale, u.shift, u.mean, u.invstd, c1, c2, u.stem_hw, ga, None, ws))
            return
        if want_w:
            b.wgrad(lambda ws: ops.rec_conv_wgrad(x, dy, ga, gb, u.k, u.k, u.s, u.p, ws, stem_hw=u.stem_hw), pixels=M, reads_slot=slot)
        if want_x:
            b.add_producer(xv, 'dgrad', lambda st: ops.rec_conv_dgrad(dy, u.wpd, xv.g(), u.k, u.k, u.s, u.p, accumulate=acc, stats=st),
                           self._dgrad_slabs(xv, u.K, u.k, u.s, u.p))

    def _mark_buckets(self, recs, side, log):
        """Data-parallel overlap (reference: DDP's autograd-hook buckets, train.py:331): cut the flat gradient buffer into ranges of
        about GRAD_BUCKET_BYTES and insert, behind the launch record that completes a range, a '@call' that tells the engine so.
        Parameters are laid out in registration (= forward) order and the backward list runs in reverse, so ranges complete from the
        end of the buffer; a range's mark sits behind the LAST record writing into it whatever the order.  Gradients this list does
        not produce (frozen parameters, the mask head's, which MaskBranchFn writes before the list runs) are final from the start."""
        store = self.grad_store
        done = {}
        for q, pos in log:
            done[id(q)] = max(done.get(id(q), -1), pos)
        items = sorted((store.offsets[id(q)], q) for q in store.params)
        marks, hi, acc, ready = [], store.numel, 0, -1
        for off, q in reversed(items):
            acc += q.numel() * 4
            ready = max(ready, done.get(id(q), -1))
            if acc >= GRAD_BUCKET_BYTES or off == 0:
                marks.append((ready, off, hi))
                hi, acc, ready = off, 0, -1
        # a range whose last writer comes later than that of a range cut after it can only go out with it: merge by position
        by_pos = {}
        for ready, a, b in marks:
            by_pos.setdefault(ready, []).append((a, b))
        self.grad_marks = []
        for pos in sorted(by_pos, reverse=True):              # insert from the back so earlier positions stay valid
            for a, b in by_pos[pos]:
                fn = (lambda a=a, b=b: self.bucket_hook(a, b, side.stream if side is not None else None) if self.bucket_hook else None)
                fn.hdy_mark = (a, b)            # bucket_marks() reads the marks back in execution order
                recs.insert(pos + 1, ('@call', fn))
                self.grad_marks.append((pos + 1, a, b))

    def bucket_marks(self):
        """the "flat gradient range [a, b) is final" marks of the backward list, in the order the list reaches them"""
        return [rec[1].hdy_mark for rec in (self.bwd or []) if rec[0] == '@call' and hasattr(rec[1], 'hdy_mark')]

    def _det_bias_tmp(self, u):
        if not hasattr(u, 'gbias_pad'):
            u.gbias_pad = self._new(u.Kp, dtype=torch.float32)
        return u.gbias_pad

    def fused_loss(self, head):
        """The hdy_det_loss call bound to this plan's logits / gradient buffers (built once)."""
        if self.loss_call is None:
            from .metayolo.models.loss import fused_criteria
            anc = [float(v) for buf in head.anchors for v in buf.anchor.flatten().tolist()]
            crit = fused_criteria(head.det_loss, head.nc)
            assert crit is not None, 'the fused loss does not cover these criteria (Detect.fused_loss_ok)'
            cls, bce, obj, _ = crit             # a FocalLoss wrapper is unwrapped: the class weights and pos_weights are its inner criterion's

            def per_class(t, default):
                if t is None:
                    return [default] * head.nc
                return [float(t)] * head.nc if t.numel() == 1 else [float(v) for v in t.flatten().tolist()]
            cw, pw = per_class(cls.weight, 1.0), per_class(bce.pos_weight, 1.0)
            obj_pw = 1.0 if obj.pos_weight is None else float(obj.pos_weight)
            self.loss_call = ops.DetLossCall([u.logits for u in self.det_units], [u.gdet for u in self.det_units], head.na, head.nc, anc,
                                             head.det_loss.balance, cw, pw, obj_pw, head.det_loss, self.loss_out, self.device)
        return self.loss_call

    def tap_features(self):
        return [self.feature(k) for k in self.tap_keys]

    def run_backward(self, gdets=None, scale=None, gtaps=None):
        """gdets: autograd's logits gradients (unfused loss), or None when the fused loss kernel already filled the plan's
        gradient buffers; then `scale` is the upstream gradient of the loss (1-element device tensor).  gtaps: gradients of the
        tapped feature maps (NCHW-shaped, or None = no outside consumer contributed in this step)."""
        if self.grad_store is not None:
            self.grad_store.before_backward()
        for i, k in enumerate(self.tap_keys):
            g = None if gtaps is None else gtaps[i]
            if g is None:
                self.outs[k].g().zero_()
            else:
                self.outs[k].g().copy_(g.permute(0, 2, 3, 1))
        if self.tap_params and not self.tap_grads_ready:
            for q in self.tap_params:
                self.grad_store.view_of(q).zero_()
        self.tap_grads_ready = False
        pre = []
        if gdets is None:
            if scale is not None:
                ops.scale_inplace(self.gdet_flat, scale.reshape(-1)[:1].float().contiguous())
        else:
            for u, g in zip(self.det_units, gdets):
                if g is None:
                    u.gdet.zero_()
                else:
                    pre.append(ops.rec_det_grad_pack(g, u.gdet, u.na, u.no))
        ops.run(pre)
        if self.mask_vals and not self.mask_grads_ready:
            for v in self.mask_vals:                 # no mask loss in this step: the branch contributes nothing
                v.g().zero_()
            for q in self.seg_h_params:
                self.grad_store.view_of(q).zero_()
        self.mask_grads_ready = False
        self._replay('bwd', self.bwd)
