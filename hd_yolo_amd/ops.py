"""Tensor-level wrappers over the C ABI (include/hdyolo.h).

torch is used here for device memory and streams only: every function takes NHWC device tensors
(shape [N, H, W, C], possibly a channel-slice view of a wider buffer), checks that they are laid out the
way the kernels assume, and builds a *launch record* `(symbol, args)` whose pointer arguments are raw
device addresses.  Records are either executed at once (`run`) or stored in a static plan
(hd_yolo_amd/plan.py) and replayed every step with no further Python-side work.
"""
import ctypes
import struct
import os
import threading

import torch

from . import _ext, _lib
from ._lib import ACT_NONE, ACT_RELU, ACT_SILU, BF16, F32, PACK_DGRAD, PACK_FWD, PACK_STEM  # noqa: F401
from .texture import OFFSETS as TEXTURE_OFFSETS  # noqa: F401  the default offsets of label_texture and of texture.texture_table

BN_EPS, BN_MOMENTUM = 1e-3, 0.03     # metayolo/models/utils_torch.py:47-49


def _rec(scope, name, args):
    """launch record = (symbol, args, tensors kept alive while the record exists)"""
    return (name, args, tuple(v for v in scope.values() if isinstance(v, torch.Tensor)) +
            tuple(t for v in scope.values() if isinstance(v, (list, tuple)) for t in v if isinstance(t, torch.Tensor)))


def dcode(dtype):
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    raise _lib.HdyError(f'unsupported arithmetic type {dtype}: use torch.float32 or torch.bfloat16')


def stat_slabs(N, H, W, C, K, R, S, stride, pad, dtype):
    """How many [2][K] statistic slabs hdy_conv_fwd writes for this layer (kernel-dependent)."""
    return _lib.query('hdy_conv_stat_slabs', N, H, W, C, K, R, S, stride, pad, dcode(dtype))


def require_gpu(t):
    if not t.is_cuda:
        raise _lib.HdyError('hd_yolo_amd runs on MI355X only: tensor is on CPU and there is no CPU fallback '
                            '(the CPU oracle under oracle/ is test infrastructure)')


def nhwc(t):
    """(ptr, N, H, W, C, pitch) of an NHWC tensor or channel-slice view."""
    require_gpu(t)
    assert t.dim() == 4 and (t.shape[3] == 1 or t.stride(3) == 1), f'not NHWC-contiguous in C: {t.shape} {t.stride()}'
    n, h, w, c = t.shape
    ld = t.stride(2)
    assert ld >= c and (h == 1 or t.stride(1) == w * ld) and (n == 1 or t.stride(0) == h * w * ld), \
        f'pixel pitch is not uniform: {t.shape} {t.stride()}'
    return t.data_ptr(), n, h, w, c, ld


def ptr(t):
    if t is None:
        return None
    require_gpu(t)
    return t.data_ptr()


def _nbytes(t):
    """byte size of a caller-owned workspace tensor (0 for None): every workspace pointer of the C ABI travels with its size"""
    return 0 if t is None else t.numel() * t.element_size()


def _workspace(nbytes, dev):
    """a 16-byte aligned workspace of at least nbytes (a sizing query's answer), as int64 words"""
    return torch.empty(((nbytes + 15) // 16 * 2,), dtype=torch.int64, device=dev)


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


class SideStream:
    """A second HIP stream for launch records that are off the critical path (weight gradients in the backward list): the
    plan brackets them with ('@fork', side, records) — they start once everything issued so far on the main stream is done —
    and ('@join', side, token) before a buffer they read is overwritten / at the end of the list."""

    def __init__(self, device):
        self.stream = torch.cuda.Stream(device=device)      # a low/high priority made no difference (18.0-18.3 ms either way)
        self.done = {}                    # token -> event recorded on the side stream after that fork's records

    def fork(self, records, token, main):
        ev = torch.cuda.Event()
        ev.record(main)
        self.stream.wait_event(ev)
        run(records, stream=self.stream.cuda_stream)
        done = torch.cuda.Event()
        done.record(self.stream)
        self.done[token] = done

    def join(self, token, main):
        done = self.done.pop(token, None)
        if done is not None:
            main.wait_event(done)
        # (a fork and its join always sit in ONE list, and a list runs either here or, compiled, through hdy_exec_run, whose events live in the
        # library: a token unknown here was never forked through this object)


# ------------------------------------------------------------------------------------------ compiled launch lists (csrc/exec.hip)
EXEC_FORK, EXEC_JOIN = _lib.CONSTANTS['HDY_EXEC_FORK'], _lib.CONSTANTS['HDY_EXEC_JOIN']
USE_EXEC = os.environ.get('HDY_EXEC', '1') != '0'        # HDY_EXEC=0: every list through the Python loop below (A/B, debugging)
_M64 = (1 << 64) - 1


def _word(v, ctype):
    """one launch argument widened to the 64-bit word hdy_exec_run expects for a parameter of ctypes type `ctype`"""
    if ctype is ctypes.c_float:
        return struct.unpack('<I', struct.pack('<f', float(v)))[0]
    if ctype is ctypes.c_double:
        return struct.unpack('<Q', struct.pack('<d', float(v)))[0]
    if v is None:
        return 0
    if isinstance(v, int):
        return v & _M64
    if isinstance(v, ctypes._SimpleCData):
        return (v.value or 0) & _M64
    return ctypes.cast(v, ctypes.c_void_p).value or 0       # ctypes array / pointer / structure reference


class Program:
    """A launch list compiled for hdy_exec_run: segments of 64-bit words (one C call each) between the list's host callbacks.  It keeps the
    records (and through them every tensor and host array whose address the words hold) alive."""

    # the library's fork events are per (device, token): every live program owns its own range of the 65536 tokens (two programs sharing events
    # could lose a fork dependency when they run on different stream pairs).  Ranges are handed out under a lock, returned by __del__, and an
    # exhausted table is an error, never a silent wrap.
    _TOKENS = 65536
    _lock = threading.Lock()
    _next_token = 0
    _free = []                          # [(base, count)] of programs that are gone

    @classmethod
    def _take_tokens(cls, n):
        with cls._lock:
            for i, (base, cnt) in enumerate(cls._free):
                if cnt >= n:
                    if cnt == n:
                        del cls._free[i]
                    else:
                        cls._free[i] = (base + n, cnt - n)
                    return base
            if cls._next_token + n > cls._TOKENS:
                raise _lib.HdyError(f'launch-list programs: all {cls._TOKENS} fork tokens are held by live programs ({n} more wanted)')
            base = cls._next_token
            cls._next_token += n
            return base

    def __del__(self):
        n = getattr(self, '_ntok', 0)
        if n:
            with Program._lock:
                # returned ranges are merged with their neighbours (and with the unissued tail), so a long run of programs of growing size —
                # tapes re-recorded every step — cannot fragment the table into ranges nobody fits
                fr = sorted(Program._free + [(self.token_base, n)])
                merged = []
                for base, cnt in fr:
                    if merged and merged[-1][0] + merged[-1][1] == base:
                        merged[-1] = (merged[-1][0], merged[-1][1] + cnt)
                    else:
                        merged.append((base, cnt))
                if merged and merged[-1][0] + merged[-1][1] == Program._next_token:
                    Program._next_token = merged.pop()[0]
                Program._free[:] = merged

    def __init__(self, records):
        lib = _lib.load()
        self.records = records
        self.nrec = len(records)        # Plan._replay recompiles when the list it was made from has changed length in place
        self.side = None
        self.segments = []              # ('words', ctypes array, count) | ('call', fn)
        words = []
        ntok = 1 + max([r[3] for r in records if r[0] == '@fork'] + [r[2] for r in records if r[0] == '@join'] + [0])
        self.token_base = Program._take_tokens(ntok)
        self._ntok = ntok

        def item(rec):
            name, args = rec[0], rec[1]
            op = lib.hdy_exec_op(name.encode())
            types = _lib.SIGNATURES[name][1]
            if op < 0 or len(args) != len(types) - 1:
                raise _lib.HdyError(f'{name} cannot be listed for hdy_exec_run ({len(args)} arguments recorded, {len(types) - 1} expected: '
                                    f'{", ".join(p for p, _ in _lib.PARAMS[name][:-1])})')
            return [op, len(args)] + [_word(v, t) for v, t in zip(args, types)]

        def flush():
            if words:
                self.segments.append(('words', (ctypes.c_ulonglong * len(words))(*words), len(words)))
                del words[:]

        for rec in records:
            name = rec[0]
            if name == '@call':
                flush()
                self.segments.append(('call', rec[1]))
            elif name in ('@fork', '@join'):
                if self.side is not None and self.side is not rec[1]:
                    raise _lib.HdyError('a launch list forks onto one side stream')
                self.side = rec[1]
                if name == '@join':
                    words.extend([EXEC_JOIN, 1, self.token_base + rec[2]])
                else:
                    body = [w for r in rec[2] for w in item(r)]       # (a host callback inside a fork: not a launch record -> KeyError above)
                    words.extend([EXEC_FORK, 2, self.token_base + rec[3], len(body)] + body)
            else:
                words.extend(item(rec))
        flush()

    def run(self):
        lib = _lib.load()
        main = stream_ptr()
        side = self.side.stream.cuda_stream if self.side is not None else None
        for seg in self.segments:
            if seg[0] == 'call':
                seg[1]()
                continue
            rc = lib.hdy_exec_run(seg[1], seg[2], main, side)
            if rc != 0:
                raise _lib.HdyError(f'hdy_exec_run failed (status {rc}): {lib.hdy_last_error().decode()}')


def run(records, stream=None):
    """Execute launch records on `stream` (default: torch's current HIP stream)."""
    lib = _lib.load()
    s = stream_ptr() if stream is None else stream
    if Tape.current is not None and stream is None:
        Tape.current.records.extend(records)
    for rec in records:
        name, args = rec[0], rec[1]
        if name[0] == '@':
            side = rec[1]
            if name == '@call':
                rec[1]()
            elif name == '@fork':
                side.fork(rec[2], rec[3], torch.cuda.current_stream())
            elif name == '@join':
                side.join(rec[2], torch.cuda.current_stream())
            continue
        rc = getattr(lib, name)(*args, s)
        if rc != 0:
            raise _lib.HdyError(f'{name} failed (status {rc}): {lib.hdy_last_error().decode()}')


# ------------------------------------------------------------------------------------------ tapes: record an eager call sequence once, replay it as one list
class Tape:
    """Records what a sequence of eager calls of THIS module launches and allocates, so that the same sequence can later be replayed
    as one compiled launch list (`Program`, one C call) over the same buffers — for call sequences whose shapes and pointers are
    fixed but which are written as ordinary eager code (hnet's segmentation branch, hd_yolo_amd/segrun.py).

        with tape:                   # first time: runs eagerly AND records
            y = some_eager_code(x)
        ...
        tape.replay()                # later: the same launches over the same buffers, no Python between them

    While a tape is active, `run()` and `_call()` append their launch records to it and `_new()` allocations are kept alive by it
    (a replay writes the same addresses, so everything the recorded code allocated must outlive the tape).  Host-side tensor
    expressions between the launches are NOT captured: code meant for a tape uses launch records for everything it does per call."""
    current = None

    def __init__(self):
        self.records, self.keep, self.prog = [], [], None

    def __enter__(self):
        assert Tape.current is None, 'tapes do not nest'
        Tape.current = self
        return self

    def __exit__(self, *exc):
        Tape.current = None
        return False

    def replay(self):
        if not USE_EXEC:
            return run(self.records)
        if self.prog is None:
            self.prog = Program(self.records)
        self.prog.run()


def _new(shape, dtype, device, zero=False):
    """torch.empty / torch.zeros that an active tape keeps alive"""
    t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=device)
    if Tape.current is not None:
        Tape.current.keep.append(t)
    return t


def _call(name, *args):
    """one launch through the C ABI on the current stream (`args` without the trailing stream); recorded by an active tape"""
    _lib.call(name, *args, stream_ptr())
    if Tape.current is not None:
        Tape.current.records.append((name, args, ()))


# ------------------------------------------------------------------------------------------ convolution
def out_dim(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def pack_alloc(K, C, R, S, stride, pad, kind, dtype, device):
    n = _lib.query('hdy_conv_pack_elems', K, C, R, S, stride, pad, kind, dcode(dtype))
    return torch.empty(n, dtype=dtype, device=device)


def rec_pack(w_a, w_b, stride, pad, kind, out, K=None):
    """Pack framework weights [K,C,R,S] fp32 (optionally two stacked along K, zero padded to K rows) into `out`."""
    K_a, C, R, S = w_a.shape
    K_b = 0 if w_b is None else w_b.shape[0]
    K = K_a + K_b if K is None else K
    assert w_a.is_contiguous() and w_a.dtype == torch.float32 and (w_b is None or (w_b.is_contiguous() and w_b.shape[1:] == w_a.shape[1:]))
    return _rec(locals(), 'hdy_conv_pack', (ptr(w_a), K_a, ptr(w_b), K_b, K, C, R, S, stride, pad, kind, dcode(out.dtype), ptr(out)))


def rec_conv_fwd(x, wp, y, K, R, S, stride, pad, scale=None, shift=None, stats=None, act=ACT_NONE, accumulate=False,
                 stem_hw=None, res=None):
    """y = act(scale*conv(x)+shift).  For the stem, x is the hdy_stem_prep buffer and stem_hw = (H, W) of the image."""
    xp, N, H, W, C, ldx = nhwc(x)
    yp, _, Ho, Wo, Ky, ldy = nhwc(y)
    stem = 0
    if stem_hw is not None:
        stem, (H, W), C = 1, stem_hw, 3
    assert Ky == K and Ho == out_dim(H, R, stride, pad) and Wo == out_dim(W, S, stride, pad), (y.shape, K, Ho, Wo)
    out_f32 = 1 if (y.dtype == torch.float32 and x.dtype == torch.bfloat16) else 0
    assert y.dtype == x.dtype or out_f32
    rp, ldr = None, 0
    if res is not None:
        rp, _, _, _, Kr, ldr = nhwc(res)
        assert Kr == K and res.dtype == y.dtype and res.shape == y.shape
    return _rec(locals(), 'hdy_conv_fwd', (xp, ldx, ptr(wp), ptr(scale), ptr(shift), rp, ldr, yp, ldy, ptr(stats), 0 if stats is None else stats.shape[0], N, H, W, C, K, R, S, stride, pad, act,
                             int(accumulate), dcode(x.dtype), out_f32, stem))


class StatRequest:
    """One producer-side BatchNorm-backward statistics request (hdy_stat_req): the producer's output channels [c0, c1) are the gradient
    of a unit whose raw conv output is `y` (an NHWC view of exactly those c1 - c0 channels); slabs: fp32 [nslabs][2][c1 - c0]."""

    def __init__(self, y, scale, shift, slabs, c0, act):
        yp, _, _, _, K, ldy = nhwc(y)
        for t in (scale, shift):
            assert t.dtype == torch.float32 and t.numel() >= K and t.stride(0) == 1
        assert slabs.dtype == torch.float32 and slabs.is_contiguous() and slabs.shape[1:] == (2, K)
        self.c = _lib.StatReq(yp, ldy, ptr(scale), ptr(shift), ptr(slabs), c0, c0 + K, act, slabs.shape[0])
        self.keep = (y, scale, shift, slabs)


def _stat_array(stats):
    arr = (_lib.StatReq * len(stats))(*[q.c for q in stats])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def conv_dgrad_stat_slabs(N, H, W, C, K, R, S, stride, pad, dtype):
    """workgroups (= statistics slabs) of the data-gradient launch of this shape; 0: it cannot serve statistics"""
    return _lib.query('hdy_conv_dgrad_stat_slabs', N, H, W, C, K, R, S, stride, pad, dcode(dtype))


def rec_conv_dgrad(dy, wp_d, dx, R, S, stride, pad, accumulate=False, stats=None):
    dyp, N, Ho, Wo, K, lddy = nhwc(dy)
    dxp, _, H, W, C, lddx = nhwc(dx)
    assert Ho == out_dim(H, R, stride, pad) and Wo == out_dim(W, S, stride, pad) and dy.dtype == dx.dtype
    if stats:
        arr, arrp = _stat_array(stats)
        keep = [t for q in stats for t in q.keep]
        return _rec(locals(), 'hdy_conv_dgrad_stats', (dyp, lddy, ptr(wp_d), dxp, lddx, N, H, W, C, K, R, S, stride, pad, int(accumulate), dcode(dy.dtype),
                                                       arrp, len(stats))) + ((arr,),)
    return _rec(locals(), 'hdy_conv_dgrad', (dyp, lddy, ptr(wp_d), dxp, lddx, N, H, W, C, K, R, S, stride, pad, int(accumulate), dcode(dy.dtype)))


def rec_bn_bwd_finalize_slabs(slabs, count, mean, invstd, dgamma, dbeta, c1, c2, accumulate=False):
    """slabs [n][2][K] of (SUM du, SUM du*y) -> dbeta, dgamma = invstd*(SUM du*y - mean*SUM du) (+)=; c1 = dbeta / count, c2 = dgamma / count"""
    n, _, K = slabs.shape
    assert slabs.is_contiguous() and c1.numel() >= K and c2.numel() >= K and mean.numel() >= K and invstd.numel() >= K
    return _rec(locals(), 'hdy_bn_bwd_finalize_slabs', (ptr(slabs), n, K, count, ptr(mean), ptr(invstd), ptr(dgamma), ptr(dbeta), int(accumulate),
                                                        ptr(c1), ptr(c2)))


def fused_1x1_stat_slabs(M, C, K, dtype):
    return _lib.query('hdy_conv1x1_bwd_fused_stat_slabs', M, C, K, dcode(dtype))


def rec_bn_act_bwd_apply(dz_a, dz_b, y, scale, shift, mean, invstd, c1, c2, dy, act=ACT_SILU):
    dap, N, H, W, Ka, ldda = nhwc(dz_a)
    dbp, lddb = None, 0
    K = Ka
    if dz_b is not None:
        dbp, _, _, _, Kb, lddb = nhwc(dz_b)
        K = Ka + Kb
    yp, _, _, _, Ky, ldy = nhwc(y)
    dyp, _, _, _, _, lddy = nhwc(dy)
    assert Ky == K and y.shape == dy.shape and y.dtype == dy.dtype == dz_a.dtype
    return _rec(locals(), 'hdy_bn_act_bwd_apply', (dap, ldda, dbp, lddb, Ka, yp, ldy, ptr(scale), ptr(shift), ptr(mean), ptr(invstd), ptr(c1), ptr(c2),
                                                  dyp, lddy, N * H * W, K, act, dcode(y.dtype)))


def wgrad_ws_bytes(N, H, W, C, K, R, S, stride, pad, dtype, stem=False):
    return _lib.query('hdy_conv_wgrad_workspace_bytes', N, H, W, C, K, R, S, stride, pad, dcode(dtype), int(stem))


def rec_conv_wgrad(x, dy, grad_a, grad_b, R, S, stride, pad, ws, accumulate=False, stem_hw=None):
    xp, N, H, W, C, ldx = nhwc(x)
    dyp, _, Ho, Wo, K, lddy = nhwc(dy)
    stem = 0
    if stem_hw is not None:
        stem, (H, W), C = 1, stem_hw, 3
    K_a = grad_a.shape[0]
    K_b = 0 if grad_b is None else grad_b.shape[0]
    assert grad_a.is_contiguous() and grad_a.dtype == torch.float32 and tuple(grad_a.shape[1:]) == (C, R, S)
    return _rec(locals(), 'hdy_conv_wgrad', (xp, ldx, dyp, lddy, N, H, W, C, K, R, S, stride, pad, ptr(grad_a), K_a, ptr(grad_b), K_b, int(accumulate),
                               ptr(ws), ws.numel() * ws.element_size(), dcode(x.dtype), stem))


def wgrad_stem_fused_ok(N, H, W, K, dtype):
    return dtype == torch.bfloat16 and bool(_lib.query('hdy_conv_wgrad_stem_fused_ok', N, H, W, K))


def rec_conv_wgrad_stem_fused(x, dz, y, scale, shift, mean, invstd, c1, c2, hw, grad_a, grad_b, ws, accumulate=False):
    """stem weight gradient straight from (dz, y): the BatchNorm / SiLU backward is applied while the tile is staged (no dy tensor)"""
    dzp, N, Ho, Wo, K, lddz = nhwc(dz)
    yp, _, _, _, _, ldy = nhwc(y)
    H, W = hw
    K_a = grad_a.shape[0]
    K_b = 0 if grad_b is None else grad_b.shape[0]
    assert dz.dtype == torch.bfloat16 and y.dtype == torch.bfloat16 and grad_a.is_contiguous() and grad_a.dtype == torch.float32
    return _rec(locals(), 'hdy_conv_wgrad_stem_fused', (ptr(x), dzp, lddz, yp, ldy, ptr(scale), ptr(shift), ptr(mean), ptr(invstd), ptr(c1), ptr(c2), N, H, W, K,
                                          ptr(grad_a), K_a, ptr(grad_b), K_b, int(accumulate), ptr(ws), ws.numel() * ws.element_size()))


ALWAYS_REPACK = os.environ.get('HDY_ALWAYS_REPACK') is not None


def _versions(tensors):
    return tuple((t.data_ptr(), t._version) for t in tensors if t is not None)


class BnEvalTable:
    """The eval-mode scale / shift of every BatchNorm of a plan in one launch (hdy_bn_eval_coeffs_batch): descriptors are built once,
    live in a small device table and are replayed before every forward (the running statistics and parameters may have changed)."""

    def __init__(self, device):
        self.device, self.descs, self.keep, self.table = device, [], [], None

    def add(self, gamma, beta, rmean, rvar, scale, shift, eps=BN_EPS):
        for t in (gamma, beta, rmean, rvar, scale, shift):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= gamma.numel()
        self.descs.append(_lib.BnEvalDesc(ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), ptr(scale), ptr(shift), gamma.numel(), float(eps)))
        self.keep += [gamma, beta, rmean, rvar, scale, shift]
        self.table = None

    def run(self, skip_unchanged=False):
        if not self.descs:
            return
        if self.table is None:
            self.table = _lib.device_table(self.descs, self.device)
            self.seen = None
        if skip_unchanged and not ALWAYS_REPACK:
            now = _versions(self.keep)
            if now == self.seen:
                return
            self.seen = now
        _lib.call('hdy_bn_eval_coeffs_batch', self.table.data_ptr(), len(self.descs), stream_ptr())


class PackTable:
    """All weight re-packing jobs of a plan as ONE launch: descriptors are built once (hdy_conv_pack_describe), live in a small
    device table, and hdy_conv_pack_run replays them after every optimizer step."""

    def __init__(self, device):
        self.device, self.descs, self.blocks, self.keep, self.table = device, [], 0, [], None

    def add(self, w_a, w_b, stride, pad, kind, out, K=None):
        K_a, C, R, S = w_a.shape
        K_b = 0 if w_b is None else w_b.shape[0]
        K = K_a + K_b if K is None else K
        assert w_a.is_contiguous() and w_a.dtype == torch.float32 and (w_b is None or (w_b.is_contiguous() and w_b.shape[1:] == w_a.shape[1:]))
        buf = (_lib.PackDesc * 4)()
        n = _lib.query('hdy_conv_pack_describe', ptr(w_a), K_a, ptr(w_b), K_b, K, C, R, S, stride, pad, kind, dcode(out.dtype), ptr(out),
                       ctypes.cast(buf, ctypes.c_void_p), self.blocks)
        if n <= 0:
            raise _lib.HdyError(f'hdy_conv_pack_describe failed: {_lib.load().hdy_last_error().decode()}')
        for i in range(n):
            d = _lib.PackDesc.from_buffer_copy(bytes(buf[i]))
            self.descs.append(d)
            self.blocks += d.nblocks
        self.keep += [w_a, w_b, out]
        self.table = None

    def run(self, skip_unchanged=False):
        """skip_unchanged (inference plans): re-pack only when a source tensor's version counter moved since the last run.  Every
        in-place write through the parameter itself (optimizer steps, load_state_dict, EMA updates on state_dict() tensors) bumps
        it; writes through `param.data` do not — after those, call model.train(); model.eval() or set HDY_ALWAYS_REPACK=1."""
        if not self.descs:
            return
        if self.table is None:
            self.table = _lib.device_table(self.descs, self.device)
            self.seen = None
        if skip_unchanged and not ALWAYS_REPACK:
            now = _versions(self.keep[0::3] + self.keep[1::3])
            if now == self.seen:
                return
            self.seen = now
        _lib.call('hdy_conv_pack_run', self.table.data_ptr(), len(self.descs), self.blocks, stream_ptr())


# ------------------------------------------------------------------------------------------ BN / act
def rec_bn_finalize(stats, mtiles, K, count, gamma, beta, rmean, rvar, scale, shift, save_mean, save_invstd,
                    eps=BN_EPS, momentum=BN_MOMENTUM, stats_ld=None, ws=None):
    """stats may be a channel slice [.., k0:k0+K] of a wider slab: stats_ld is the slab's channel count."""
    return _rec(locals(), 'hdy_bn_finalize', (ptr(stats), K if stats_ld is None else stats_ld, mtiles, K, count, ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), eps, momentum, ptr(scale),
                                ptr(shift), ptr(save_mean), ptr(save_invstd), ptr(ws), _nbytes(ws)))


def rec_bn_finalize_pair(stats, mtiles, K, Ka, count, bn_a, bn_b, scale, shift, save_mean, save_invstd, eps=BN_EPS, momentum=BN_MOMENTUM, ws=None):
    """One finalize for the two BatchNorms of a merged cv1 | cv2 convolution: bn_a / bn_b = (gamma, beta, running_mean, running_var)."""
    ga, ba, rma, rva = bn_a
    gb, bb, rmb, rvb = bn_b
    return _rec(locals(), 'hdy_bn_finalize_pair', (ptr(stats), K, mtiles, K, Ka, count, ptr(ga), ptr(ba), ptr(rma), ptr(rva), ptr(gb), ptr(bb), ptr(rmb),
                                     ptr(rvb), eps, momentum, ptr(scale), ptr(shift), ptr(save_mean), ptr(save_invstd), ptr(ws), _nbytes(ws)))


def rec_bn_slab_sums(slabs, nslabs, K, count, sums):
    """SyncBatchNorm: fp32 slabs [nslabs][2][K] -> sums = 2K + 1 doubles [SUM | SUM2 | count] (the buffer the caller all-reduces)."""
    assert sums.dtype == torch.float64 and sums.numel() == 2 * K + 1 and sums.is_contiguous()
    return _rec(locals(), 'hdy_bn_slab_sums', (ptr(slabs), K, nslabs, K, count, ptr(sums)))


def rec_bn_finalize_sums(sums, Ktot, k0, K, Ka, bn_a, bn_b, scale, shift, save_mean, save_invstd, eps=BN_EPS, momentum=BN_MOMENTUM):
    """finalize of the channels [k0, k0 + K) of an all-reduced sums block over Ktot channels; bn_b: the second module of a pair (Ka < K)"""
    ga, ba, rma, rva = bn_a
    gb, bb, rmb, rvb = bn_b if bn_b is not None else (None, None, None, None)
    base = sums.data_ptr()
    return _rec(locals(), 'hdy_bn_finalize_sums', (base + 8 * k0, Ktot, base + 16 * Ktot, K, Ka, ptr(ga), ptr(ba), ptr(rma), ptr(rva), ptr(gb), ptr(bb), ptr(rmb),
                                     ptr(rvb), eps, momentum, ptr(scale), ptr(shift), ptr(save_mean), ptr(save_invstd)))


def rec_bn_bwd_coeffs_sums(sums, K, c1, c2):
    return _rec(locals(), 'hdy_bn_bwd_coeffs_sums', (ptr(sums), K, ptr(c1), ptr(c2)))


def rec_bn_eval_coeffs(gamma, beta, rmean, rvar, scale, shift, eps=BN_EPS):
    return _rec(locals(), 'hdy_bn_eval_coeffs', (ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), eps, gamma.numel(), ptr(scale), ptr(shift)))


def rec_bn_act_fwd(y, scale, shift, z, res=None, act=ACT_SILU):
    yp, N, H, W, K, ldy = nhwc(y)
    zp, _, _, _, Kz, ldz = nhwc(z)
    assert Kz == K and z.shape == y.shape and z.dtype == y.dtype
    rp, ldr = None, 0
    if res is not None:
        rp, _, _, _, Kr, ldr = nhwc(res)
        assert Kr == K and res.dtype == y.dtype
    return _rec(locals(), 'hdy_bn_act_fwd', (yp, ldy, ptr(scale), ptr(shift), rp, ldr, zp, ldz, N * H * W, K, act, dcode(y.dtype)))


def rec_bn_act_fwd_pair(y, scale, shift, z_a, z_b, act=ACT_SILU):
    """z_a = channels [0, Ka), z_b = the rest: the two outputs of a merged cv1 | cv2 unit (different buffers / pitches)."""
    yp, N, H, W, K, ldy = nhwc(y)
    zap, _, _, _, Ka, ldza = nhwc(z_a)
    zbp, _, _, _, Kb, ldzb = nhwc(z_b)
    assert Ka + Kb == K and z_a.dtype == z_b.dtype == y.dtype and z_a.shape[:3] == z_b.shape[:3] == y.shape[:3]
    return _rec(locals(), 'hdy_bn_act_fwd_pair', (yp, ldy, ptr(scale), ptr(shift), zap, ldza, zbp, ldzb, Ka, N * H * W, K, act, dcode(y.dtype)))


def rec_bn_act_bwd_pair(dz_a, dz_b, y, scale, shift, mean, invstd, dy, dgamma_a, dbeta_a, dgamma_b, dbeta_b, ws, accumulate=False, act=ACT_SILU):
    dap, N, H, W, Ka, ldda = nhwc(dz_a)
    dbp, _, _, _, Kb, lddb = nhwc(dz_b)
    yp, _, _, _, K, ldy = nhwc(y)
    dyp, lddy = None, 0
    if dy is not None:                                 # None: statistics only (the fused 1x1 backward applies them)
        dyp, _, _, _, _, lddy = nhwc(dy)
        assert y.shape == dy.shape and y.dtype == dy.dtype
    assert Ka + Kb == K and dz_a.dtype == dz_b.dtype == y.dtype and ws.numel() >= bn_bwd_ws_floats(N * H * W, K)
    return _rec(locals(), 'hdy_bn_act_bwd_pair', (dap, ldda, dbp, lddb, Ka, yp, ldy, ptr(scale), ptr(shift), ptr(mean), ptr(invstd), dyp, lddy, ptr(dgamma_a),
                                    ptr(dbeta_a), ptr(dgamma_b), ptr(dbeta_b), int(accumulate), N * H * W, K, act, dcode(dz_a.dtype), ptr(ws), _nbytes(ws)))


def bn_bwd_blocks(M):
    return _lib.query('hdy_bn_bwd_blocks', M)


def bn_bwd_ws_floats(M, K):
    return _lib.query('hdy_bn_bwd_workspace_bytes', M, K) // 4


def rec_bn_act_bwd(dz, y, scale, shift, mean, invstd, dy, dgamma, dbeta, ws, accumulate=False, act=ACT_SILU):
    dzp, N, H, W, K, lddz = nhwc(dz)
    yp, _, _, _, _, ldy = nhwc(y)
    dyp, lddy = None, 0
    if dy is not None:
        dyp, _, _, _, _, lddy = nhwc(dy)
        assert y.shape == dy.shape and y.dtype == dy.dtype
    assert dz.shape == y.shape and dz.dtype == y.dtype and ws.numel() >= bn_bwd_ws_floats(N * H * W, K)
    return _rec(locals(), 'hdy_bn_act_bwd', (dzp, lddz, yp, ldy, ptr(scale), ptr(shift), ptr(mean), ptr(invstd), dyp, lddy, ptr(dgamma), ptr(dbeta),
                               int(accumulate), N * H * W, K, act, dcode(dz.dtype), ptr(ws), _nbytes(ws)))


def bn_bwd_coeffs(ws, M, K):
    """(c1, c2) views of the BatchNorm-backward workspace that hdy_bn_act_bwd's finalize stage fills"""
    o = _lib.query('hdy_bn_bwd_blocks', M) * 2 * K
    return ws[o:o + K], ws[o + K:o + 2 * K]


def fused_1x1_ok(C, K, dtype):
    return bool(_lib.query('hdy_conv1x1_bwd_fused_ok', C, K, dcode(dtype)))


def fused_1x1_ws_bytes(M, C, K):
    return _lib.query('hdy_conv1x1_bwd_fused_workspace_bytes', M, C, K)


def rec_conv1x1_bwd_fused(dz_a, dz_b, y, scale, shift, mean, invstd, c1, c2, x, wp_d, dx, grad_a, grad_b, ws, accumulate_dx=False, stats=None):
    """One pass: dy from (dz, y, BatchNorm coefficients) -> dx (+)= dy*W and grad_a / grad_b = dy^T * x.  dx / grad_a may be None."""
    dap, N, H, W, Ka, ldda = nhwc(dz_a)
    dbp, lddb = None, 0
    K = Ka
    if dz_b is not None:
        dbp, _, _, _, Kb, lddb = nhwc(dz_b)
        K = Ka + Kb
    yp, _, _, _, Ky, ldy = nhwc(y)
    xp, _, _, _, C, ldx = nhwc(x)
    assert Ky == K and y.shape[:3] == x.shape[:3] == dz_a.shape[:3] and y.dtype == x.dtype == dz_a.dtype == torch.bfloat16
    dxp, lddx = None, 0
    if dx is not None:
        dxp, _, _, _, Cd, lddx = nhwc(dx)
        assert Cd == C and dx.dtype == x.dtype and dx.shape[:3] == x.shape[:3]
    K_a = 0 if grad_a is None else grad_a.shape[0]
    K_b = 0 if grad_b is None else grad_b.shape[0]
    assert grad_a is None or (grad_a.is_contiguous() and grad_a.dtype == torch.float32 and tuple(grad_a.shape[1:]) == (C, 1, 1))
    args = (dap, ldda, dbp, lddb, Ka, yp, ldy, ptr(scale), ptr(shift), ptr(mean), ptr(invstd), ptr(c1), ptr(c2), xp, ldx, ptr(wp_d), dxp, lddx,
            int(accumulate_dx), ptr(grad_a), K_a, ptr(grad_b), K_b, 0, N * H * W, C, K, ptr(ws), ws.numel() * ws.element_size(), dcode(x.dtype))
    if stats:
        arr, arrp = _stat_array(stats)
        keep = [t for q in stats for t in q.keep]
        return _rec(locals(), 'hdy_conv1x1_bwd_fused_stats', args + (arrp, len(stats))) + ((arr,),)
    return _rec(locals(), 'hdy_conv1x1_bwd_fused', args)


def rec_copy_f32(src, dst):
    """dst[:] = src[:] (contiguous fp32, same length) as a list item: a host-side tensor copy would split a compiled launch list"""
    assert src.dtype == dst.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel() > 0
    return _rec(locals(), 'hdy_copy_f32', (ptr(src), ptr(dst), src.numel()))


def rec_colsum(dz, out, ws, accumulate=False):
    dzp, N, H, W, K, lddz = nhwc(dz)
    assert out.dtype == torch.float32 and out.numel() >= K and ws.numel() >= bn_bwd_ws_floats(N * H * W, K)
    return _rec(locals(), 'hdy_colsum', (dzp, lddz, N * H * W, K, ptr(out), int(accumulate), dcode(dz.dtype), ptr(ws), _nbytes(ws)))


def rec_det_grad_pack(g, out, na, no):
    """g: fp32 gradient of the logits view (B, na, ny, nx, no), any strides -> out NHWC [B, ny, nx, ld]."""
    require_gpu(g)
    B, na_, ny, nx, no_ = g.shape
    assert (na_, no_) == (na, no) and g.dtype == torch.float32
    op, _, _, _, _, ldo = nhwc(out)
    assert out.shape[:3] == (B, ny, nx) and out.is_contiguous()
    return _rec(locals(), 'hdy_det_grad_pack', (g.data_ptr(), g.stride(0), g.stride(1), g.stride(2), g.stride(3), g.stride(4), op,
                                                out.shape[3], B, na, ny, nx, no, dcode(out.dtype)))


def rec_add_inplace(out, a):
    op, N, H, W, K, ldo = nhwc(out)
    ap, _, _, _, _, lda = nhwc(a)
    assert out.shape == a.shape and out.dtype == a.dtype
    return _rec(locals(), 'hdy_add_inplace', (op, ldo, ap, lda, N * H * W, K, dcode(out.dtype)))


# ------------------------------------------------------------------------------------------ pool / upsample / layout
def rec_sppf_pool_fwd(x, y1, y2, y3, idx=None):
    xp, N, H, W, C, ld = nhwc(x)
    for t in (y1, y2, y3):
        assert nhwc(t)[5] == ld and t.shape == x.shape
    i1, i2, i3 = (None, None, None) if idx is None else idx
    return _rec(locals(), 'hdy_sppf_pool_fwd', (xp, ptr(y1), ptr(y2), ptr(y3), ld, ptr(i1), ptr(i2), ptr(i3), N, H, W, C, dcode(x.dtype)))


def rec_sppf_pool_bwd(g0, g1, g2, g3, idx, dx):
    gp, N, H, W, C, ldg = nhwc(g0)
    for t in (g1, g2, g3):
        assert nhwc(t)[5] == ldg and t.shape == g0.shape
    dxp, _, _, _, _, lddx = nhwc(dx)
    return _rec(locals(), 'hdy_sppf_pool_bwd', (gp, ptr(g1), ptr(g2), ptr(g3), ldg, ptr(idx[0]), ptr(idx[1]), ptr(idx[2]), dxp, lddx, N, H, W, C,
                                  dcode(g0.dtype)))


def rec_upsample_fwd(x, y):
    xp, N, H, W, C, ldx = nhwc(x)
    yp, _, H2, W2, _, ldy = nhwc(y)
    assert H2 == 2 * H and W2 == 2 * W and y.shape[3] == C
    return _rec(locals(), 'hdy_upsample2x_fwd', (xp, ldx, yp, ldy, N, H, W, C, dcode(x.dtype)))


def rec_upsample_bwd(dy, dx, accumulate=False):
    dxp, N, H, W, C, lddx = nhwc(dx)
    dyp, _, H2, W2, _, lddy = nhwc(dy)
    assert H2 == 2 * H and W2 == 2 * W
    return _rec(locals(), 'hdy_upsample2x_bwd', (dyp, lddy, dxp, lddx, N, H, W, C, int(accumulate), dcode(dx.dtype)))


def rec_stem_prep(img, out, pad=2):
    require_gpu(img)
    B, C, H, W = img.shape
    assert C == 3 and img.dtype == torch.float32 and img.is_contiguous()
    assert tuple(out.shape) == (B, H + 2 * pad, W + 2 * pad, 4) and out.is_contiguous()
    return _rec(locals(), 'hdy_stem_prep', (img.data_ptr(), out.data_ptr(), B, H, W, pad, dcode(out.dtype)))


def rec_nchw_to_nhwc(src, dst):
    require_gpu(src)
    N, C, H, W = src.shape
    assert src.dtype == torch.float32 and src.is_contiguous()
    dp, _, _, _, Cd, ldd = nhwc(dst)
    assert Cd == C
    return _rec(locals(), 'hdy_nchw_to_nhwc', (src.data_ptr(), dp, ldd, N, C, H, W, dcode(dst.dtype)))


# ------------------------------------------------------------------------------------------ whole-slide inference from an 8-bit slide
def slide_u8(slide):
    """(ptr, row pitch in bytes, pixel_bytes, H, W) of an 8-bit slide as readers deliver it: a CUDA uint8 tensor (H, W, 3) RGB or
    (H, W, 4) RGBA with stride(2) == 1, stride(1) == C and any row stride (a crop of a larger slide is a view, not a copy)."""
    if not isinstance(slide, torch.Tensor) or slide.dtype != torch.uint8:
        raise _lib.HdyError(f'8-bit slide: a torch.uint8 tensor is expected, got {getattr(slide, "dtype", type(slide).__name__)}')
    require_gpu(slide)
    if slide.dim() != 3 or slide.shape[2] not in (3, 4):
        raise _lib.HdyError(f'8-bit slide: shape (H, W, 3) RGB or (H, W, 4) RGBA is expected (pixels interleaved, as slide readers deliver '
                            f'them), got {tuple(slide.shape)}')
    H, W, C = slide.shape
    if H == 0 or W == 0:
        raise _lib.HdyError(f'8-bit slide: empty slide {tuple(slide.shape)}')
    if slide.stride(2) != 1 or slide.stride(1) != C or (H > 1 and slide.stride(0) < W * C):
        raise _lib.HdyError(f'8-bit slide: pixels must be interleaved and rows dense (stride(2) == 1, stride(1) == {C}, any row stride >= '
                            f'{W * C}), got strides {tuple(slide.stride())}')
    return slide.data_ptr(), int(slide.stride(0)) if H > 1 else W * C, C, H, W


def slide_origins(origins, device):
    """the device table of tile origins, int32 [n][2] = (x0, y0): uploaded once per slide"""
    t = torch.as_tensor(origins, dtype=torch.int32).reshape(-1, 2).contiguous()
    return t.to(device)


def _origin_table(origins):
    require_gpu(origins)
    assert origins.dtype == torch.int32 and origins.dim() == 2 and origins.shape[1] == 2 and origins.is_contiguous(), 'origins: int32 [n][2]'
    return origins.data_ptr(), origins.shape[0]


def rec_slide_tiles(slide, origins, first, count, out, pad=2):
    """Launch record (next to rec_stem_prep / rec_nchw_to_nhwc): tiles [first, first + count) of the 8-bit slide into `out`, either the
    contiguous stem buffer (count, th + 2 pad, tw + 2 pad, 4) or a pitched NHWC view (count, th, tw, 3) of a wider buffer (pad = 0)."""
    sp, pitch, pb, H, W = slide_u8(slide)
    op_, n = _origin_table(origins)
    require_gpu(out)
    assert out.dim() == 4 and out.shape[0] == count, (tuple(out.shape), count)
    if out.is_contiguous() and out.shape[3] == 4:
        th, tw, ldd = out.shape[1] - 2 * pad, out.shape[2] - 2 * pad, 0
        elems = out.numel()
    else:
        _, _, th, tw, C, ldd = nhwc(out)
        assert C == 3 and pad == 0, 'a pitched NHWC input takes the 3 colour channels and no frame'
        elems = count * th * tw * ldd
    return _rec(locals(), 'hdy_slide_tiles_u8', (sp, pitch, pb, H, W, op_, n, int(first), int(count), out.data_ptr(), elems, th, tw, pad, ldd,
                                                 dcode(out.dtype)))


def slide_append(boxes, scores, labels, n_keep, origins, first, out_boxes, out_scores, out_labels, cursor):
    """Append a batch's compacted single-label detections (det_outputs) to the slide-wide arrays at the device cursor (int32 [2]: rows,
    overflow flag), each box shifted by its tile's origin (hdy_slide_append).  No synchronisation."""
    op_, n = _origin_table(origins)
    B = n_keep.shape[0]
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.dim() == 2 and boxes.shape[1] == 4
    assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.dim() == 1 and labels.dtype == torch.int64 and labels.is_contiguous() \
        and labels.dim() == 1, 'single-label detections only (multi-label rows keep the Python merge)'
    assert scores.shape[0] == labels.shape[0] == boxes.shape[0] and n_keep.dtype == torch.int32 and n_keep.is_contiguous()
    cap = out_boxes.shape[0]
    assert out_boxes.dtype == torch.float32 and out_boxes.is_contiguous() and tuple(out_boxes.shape) == (cap, 4)
    assert out_scores.dtype == torch.float32 and out_scores.is_contiguous() and tuple(out_scores.shape) == (cap,)
    assert out_labels.dtype == torch.int64 and out_labels.is_contiguous() and tuple(out_labels.shape) == (cap,)
    assert cursor.dtype == torch.int32 and cursor.is_contiguous() and cursor.numel() == 2
    _call('hdy_slide_append', ptr(boxes), ptr(scores), ptr(labels), ptr(n_keep), B, boxes.shape[0], op_, n, int(first), ptr(out_boxes),
          ptr(out_scores), ptr(out_labels), cap, ptr(cursor))


def slide_tissue(slide, origins, th, tw, background=220):
    """int32 [n] device tensor: per tile of the origin table, the pixels of its th x tw window (clipped to the slide) that are not
    background — background: min(R, G, B) >= `background` (hdy_slide_tissue_u8; this rule is this project's, the reference has none)."""
    sp, pitch, pb, H, W = slide_u8(slide)
    op_, n = _origin_table(origins)
    counts = torch.empty((n,), dtype=torch.int32, device=slide.device)
    _call('hdy_slide_tissue_u8', sp, pitch, pb, H, W, op_, n, int(th), int(tw), int(background), counts.data_ptr(), n)
    return counts


# ------------------------------------------------------------------------------------------ stain counts and recolouring (csrc/stain.hip)
STAIN_MAX_BINS, STAIN_MAX_TONE = _ext.PIXEL_CONSTANTS['HDY_STAIN_MAX_BINS'], _ext.PIXEL_CONSTANTS['HDY_STAIN_MAX_TONE']
STAIN_ANGLE_ENTRY_BOUND = 2466 << _ext.PIXEL_CONSTANTS['HDY_STAIN_OD_SHIFT']      # |entry| of stain_angles' table: q(0) projected on a unit vector


def _stain_window(who, slide, window):
    """(the slide's arguments, the window's) of a stain pass: window = (x0, y0, w, h), None = the whole slide"""
    sp, pitch, pb, H, W = slide_u8(slide)
    x0, y0, w, h = (0, 0, W, H) if window is None else (int(v) for v in window)
    if x0 < 0 or y0 < 0 or w < 1 or h < 1 or x0 + w > W or y0 + h > H:
        raise _lib.HdyError(f'{who}: the window ({x0}, {y0}) + {w} x {h} leaves the slide of {W} x {H} pixels')
    return (sp, pitch, pb, H, W), (x0, y0, w, h)


def _stain_table(who, t, name, shape, dev, dtype=torch.int32):
    require_gpu(t)
    if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev:
        raise _lib.HdyError(f'{who}: {name} must be a {dtype} {shape} tensor on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}')
    return t.contiguous()


def _stain_outputs(who, out, shapes, dev):
    """the int64 outputs of a counting pass: new tensors, or the caller's (`out`, one tensor or a tuple), which the pass overwrites whole"""
    if out is None:
        return tuple(torch.empty(s, dtype=torch.int64, device=dev) for s in shapes)
    out = (out,) if isinstance(out, torch.Tensor) else tuple(out)
    if len(out) != len(shapes) or any(t.dtype != torch.int64 or tuple(t.shape) != s or t.device != dev or not t.is_contiguous()
                                      for t, s in zip(out, shapes)):
        raise _lib.HdyError(f'{who}: out must be contiguous int64 of shape {" and ".join(str(s) for s in shapes)} on {dev}')
    return out


def _stain_count(who, name, slide, window, step, background, table, cells, outs):
    """one counting pass: `table` then the (tensor, ...) outputs with their sizes, then a workspace of HDY_STAIN_MAX_BLOCKS slabs of `cells`"""
    sl, win = _stain_window(who, slide, window)
    if int(step) < 1:
        raise _lib.HdyError(f'{who}: step={step} must be at least 1')
    ws = _workspace(_ext.PIXEL_CONSTANTS['HDY_STAIN_MAX_BLOCKS'] * cells * 8, slide.device)
    args = [v for o in outs for v in (o.data_ptr(), o.numel())]
    _ext.call(name, *sl, *win, int(step), int(background), *table, *args, ws.data_ptr(), _nbytes(ws), stream_ptr())


def stain_moments(slide, od, window=None, step=1, background=220, out=None):
    """int64 (10,) device tensor: n, the sums of the optical densities qR, qG, qB = od[value] and of their six products over the tissue
    pixels (min(R, G, B) < background) of the window's every `step`-th pixel (hdy_stain_moments_u8, include/hdyolo_stain.h).  od: int32
    (256,), hd_yolo_amd.stain.od_table().  Integer sums: the same input gives the same bits.  out (here and in stain_angles / stain_levels): the
    caller's output tensors instead of new ones; every element is written."""
    who = 'stain_moments'
    od = _stain_table(who, od, 'od', (256,), slide.device)
    sums, = _stain_outputs(who, out, [(10,)], slide.device)
    _stain_count(who, 'hdy_stain_moments_u8', slide, window, step, background, (od.data_ptr(), 256), 10, (sums,))
    return sums


def stain_angles(slide, lut, A, window=None, step=1, background=220, out=None):
    """(hist int64 (A,), skipped int64 (1,)): per tissue pixel p_k = (lut[k][0][R] + lut[k][1][G] + lut[k][2][B]) >> 4, k = 0, 1; p_0 <= 0 is
    skipped, otherwise bin floor(A (s + p_1) / (2 s)), s = p_0 + |p_1|, monotone in atan2(p_1, p_0) (hdy_stain_angles_u8).  lut: int32
    (2, 3, 256), hd_yolo_amd.stain.plane_lut.  The table's bound (|entry| <= 2^10 * 2466, under which the pass's 32-bit product is exact) is
    checked here: one value is read back."""
    who = 'stain_angles'
    A = int(A)
    if not 1 <= A <= STAIN_MAX_BINS:
        raise _lib.HdyError(f'{who}: A={A} outside [1, {STAIN_MAX_BINS}]')
    lut = _stain_table(who, lut, 'lut', (2, 3, 256), slide.device)
    top = int(lut.abs().max())
    if top > STAIN_ANGLE_ENTRY_BOUND:
        raise _lib.HdyError(f'{who}: a table entry of magnitude {top} passes 2^10 * 2466 = {STAIN_ANGLE_ENTRY_BOUND}: A (s + p_1) could pass 2^32')
    hist, skipped = _stain_outputs(who, out, [(A,), (1,)], slide.device)
    _stain_count(who, 'hdy_stain_angles_u8', slide, window, step, background, (lut.data_ptr(), lut.numel(), A), A + 1, (hist, skipped))
    return hist, skipped


def stain_levels(slide, lut, B, window=None, step=1, background=220, out=None):
    """int64 (2, B): per stain s the histogram of level_s = clamp((lut[s][0][R] + lut[s][1][G] + lut[s][2][B]) >> 16, 0, B - 1) over the tissue
    pixels: the level rule of label_texture over the whole window (hdy_stain_levels_u8).  lut: int32 (2, 3, 256), hd_yolo_amd.stain.level_lut."""
    who = 'stain_levels'
    B = int(B)
    if not 1 <= B <= STAIN_MAX_BINS:
        raise _lib.HdyError(f'{who}: B={B} outside [1, {STAIN_MAX_BINS}]')
    lut = _stain_table(who, lut, 'lut', (2, 3, 256), slide.device)
    hist, = _stain_outputs(who, out, [(2, B)], slide.device)
    _stain_count(who, 'hdy_stain_levels_u8', slide, window, step, background, (lut.data_ptr(), lut.numel(), B), 2 * B, (hist,))
    return hist


def stain_apply(slide, lut, tone, out=None, window=None):
    """The slide recoloured: out_c = tone[clamp((lut[c][0][R] + lut[c][1][G] + lut[c][2][B]) >> 16, 0, T - 1)] for every pixel of the window,
    background included (hdy_stain_apply_u8).  lut int32 (3, 3, 256) and tone uint8 (T,): hd_yolo_amd.stain.normalizer.  out: None (a new
    slide of the same shape; outside a window it is a copy of the input), the slide itself (in place) or another 8-bit slide of the same
    H x W with 3 or 4 bytes per pixel (a fourth byte is the input's, or 255)."""
    who = 'stain_apply'
    sl, win = _stain_window(who, slide, window)
    lut = _stain_table(who, lut, 'lut', (3, 3, 256), slide.device)
    T = int(tone.numel())
    if not 1 <= T <= STAIN_MAX_TONE:
        raise _lib.HdyError(f'{who}: a tone table of {T} entries (1 .. {STAIN_MAX_TONE})')
    tone = _stain_table(who, tone, 'tone', (T,), slide.device, torch.uint8)
    if out is None:
        out = torch.empty_like(slide, memory_format=torch.contiguous_format) if window is None else slide.clone(memory_format=torch.contiguous_format)
    dp, dpitch, dpb, dH, dW = slide_u8(out)
    if (dH, dW) != sl[3:] or out.device != slide.device:
        raise _lib.HdyError(f'{who}: out is {dW} x {dH} pixels on {out.device}, the slide {sl[4]} x {sl[3]} on {slide.device}')
    _ext.call('hdy_stain_apply_u8', *sl, *win, dp, dpitch, dpb, lut.data_ptr(), lut.numel(), tone.data_ptr(), T, T, stream_ptr())
    return out


# ------------------------------------------------------------------------------------------ training augmentation from an 8-bit tile bank
AUG_CELL_BYTES = _lib.CONSTANTS['HDY_AUG_CELL_BYTES']


def _tile_bank_u8(tiles):
    """(ptr, tile stride, row pitch (bytes), pixel_bytes, n, H, W) of a bank: a CUDA uint8 tensor (n, H, W, 3 | 4) with interleaved pixels,
    dense rows and any row / tile stride (a crop of a larger bank is a view, not a copy)."""
    if not isinstance(tiles, torch.Tensor) or tiles.dtype != torch.uint8:
        raise _lib.HdyError(f'tile bank: a torch.uint8 tensor is expected, got {getattr(tiles, "dtype", type(tiles).__name__)}')
    require_gpu(tiles)
    if tiles.dim() != 4 or tiles.shape[3] not in (3, 4) or 0 in tiles.shape:
        raise _lib.HdyError(f'tile bank: shape (n, H, W, 3) RGB or (n, H, W, 4) RGBA is expected, got {tuple(tiles.shape)}')
    n, H, W, C = tiles.shape
    pitch = int(tiles.stride(1)) if H > 1 else W * C
    stride = int(tiles.stride(0)) if n > 1 else (H - 1) * pitch + W * C
    if tiles.stride(3) != 1 or tiles.stride(2) != C or pitch < W * C or stride < (H - 1) * pitch + W * C:
        raise _lib.HdyError(f'tile bank: pixels must be interleaved and rows dense, got strides {tuple(tiles.stride())}')
    return tiles.data_ptr(), stride, pitch, C, n, H, W


def _cell_table(cells, crop, k):
    require_gpu(cells)
    assert cells.dtype == torch.uint8 and cells.dim() == 2 and cells.shape[1] == AUG_CELL_BYTES and cells.is_contiguous(), \
        f'cell table: uint8 [B * k * k][{AUG_CELL_BYTES}]'
    assert crop.dtype == torch.int32 and crop.dim() == 2 and crop.shape[1] == 2 and crop.is_contiguous() and crop.is_cuda, 'crop: int32 [B][2]'
    return cells.data_ptr(), cells.shape[0], crop.data_ptr(), crop.shape[0]


def augment_tiles(tiles, cells, crop, out, patch, k, cval):
    """The augmented batch (hdy_augment_tiles_u8): `out` (B, 3, S, S) fp32 / bf16 contiguous, from the bank `tiles`, the device cell table
    uint8 (B * k * k, AUG_CELL_BYTES) and crop offsets int32 (B, 2) that hd_yolo_amd.augment.cell_tables packs.  No synchronisation."""
    bp, stride, pitch, pb, n, H, W = _tile_bank_u8(tiles)
    cp, n_cells, rp, B = _cell_table(cells, crop, k)
    require_gpu(out)
    assert out.dim() == 4 and out.shape[0] == B and out.shape[1] == 3 and out.shape[2] == out.shape[3] and out.is_contiguous(), tuple(out.shape)
    _call('hdy_augment_tiles_u8', bp, stride, pitch, pb, n, H, W, cp, n_cells, rp, B, int(patch), int(k), int(out.shape[2]), int(cval),
          out.data_ptr(), out.numel(), dcode(out.dtype))
    return out


def augment_boxes(bank_boxes, bank_labels, offsets, n_boxes, cells, crop, patch, k, img_size, out_boxes, out_labels, out_img, counts, overflow):
    """The batch's transformed targets (hdy_augment_boxes): compact normalised xyxy rows in (image, cell, source) order into out_boxes
    (cap, 4) / out_labels int64 (cap,) / out_img fp32 (cap,), rows per image into counts int32 (B,), overflow int32 (1,) = 1 when more than
    cap rows were kept.  n_boxes: rows of the bank's box array that are annotations.  No synchronisation."""
    cp, n_cells, rp, B = _cell_table(cells, crop, k)
    cap = out_boxes.shape[0]
    assert bank_boxes.dtype == torch.float32 and bank_boxes.is_contiguous() and bank_boxes.dim() == 2 and bank_boxes.shape[1] == 4
    assert bank_labels.dtype == torch.int64 and bank_labels.is_contiguous() and offsets.dtype == torch.int64 and offsets.is_contiguous()
    assert 0 <= n_boxes <= bank_boxes.shape[0] and bank_labels.shape[0] >= n_boxes
    assert out_boxes.dtype == torch.float32 and out_boxes.is_contiguous() and tuple(out_boxes.shape) == (cap, 4)
    assert out_labels.dtype == torch.int64 and out_labels.is_contiguous() and tuple(out_labels.shape) == (cap,)
    assert out_img.dtype == torch.float32 and out_img.is_contiguous() and tuple(out_img.shape) == (cap,)
    assert counts.dtype == torch.int32 and counts.is_contiguous() and overflow.dtype == torch.int32 and overflow.numel() >= 1
    _call('hdy_augment_boxes', ptr(bank_boxes), ptr(bank_labels), ptr(offsets), offsets.shape[0] - 1, int(n_boxes), cp, n_cells, rp, B,
          int(patch), int(k), int(img_size), ptr(out_boxes), ptr(out_labels), ptr(out_img), cap, ptr(counts), counts.numel(), ptr(overflow))


AUG_MASK_SIDE = 28
AUG_MASK_REC_BYTES = 32


def _instance_map(instances, has_mask, offsets):
    """(ptr, n, H, W) of an instance map: a CUDA int16 / uint16 tensor (n, H, W), dense (the uint16 bits of TileBank.instances)"""
    require_gpu(instances)
    assert instances.dtype in (torch.int16, torch.uint16) and instances.dim() == 3 and instances.is_contiguous(), 'instance map: 16-bit (n, H, W), dense'
    assert instances.shape[0] == offsets.shape[0] - 1, 'instance map: one plane per tile of the bank'
    assert has_mask.dtype == torch.uint8 and has_mask.is_contiguous() and has_mask.is_cuda and has_mask.dim() == 1
    assert offsets.dtype == torch.int64 and offsets.is_contiguous()
    return (instances.data_ptr(),) + tuple(instances.shape)


def _mask_workspace(ws, n_cells, pitch):
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.is_cuda and 1 <= pitch <= 0xFFFF
    return ws.data_ptr(), ws.numel()


def augment_mask_workspace_bytes(n_cells, pitch):
    """bytes of the extents workspace of a batch of n_cells cells whose tiles hold at most `pitch` boxes"""
    return int(n_cells) * int(pitch) * AUG_MASK_REC_BYTES


def augment_mask_extents(instances, bank_boxes, has_mask, offsets, n_boxes, cells, crop, patch, k, img_size, ws, pitch):
    """Per candidate (cell, object of the cell's tile) the extents record of its warped mask (hdy_augment_mask_extents): member count, umin,
    umax, vmin, vmax, pixels inside the image — int32 [n_cells][pitch][8] into the uint8 workspace `ws`.  has_mask uint8 (>= n_boxes,);
    pitch: at least the bank's largest box count per tile.  No synchronisation."""
    cp, n_cells, rp, B = _cell_table(cells, crop, k)
    ip, n, H, W = _instance_map(instances, has_mask, offsets)
    assert bank_boxes.dtype == torch.float32 and bank_boxes.is_contiguous() and bank_boxes.dim() == 2 and bank_boxes.shape[1] == 4
    assert 0 <= n_boxes <= bank_boxes.shape[0] and has_mask.shape[0] >= n_boxes
    wp, wbytes = _mask_workspace(ws, n_cells, pitch)
    _call('hdy_augment_mask_extents', ip, n, H, W, ptr(bank_boxes), ptr(has_mask), ptr(offsets), int(n_boxes), cp, n_cells, rp, B, int(patch), int(k),
          int(img_size), wp, wbytes, int(pitch))
    return ws


def augment_boxes_masks(bank_boxes, bank_labels, has_mask, offsets, n_boxes, cells, crop, patch, k, img_size, ws, pitch, out_boxes, out_labels,
                        out_img, out_ref, counts, overflow, total):
    """augment_boxes for a bank with an instance map (hdy_augment_boxes_masks): a row with has_mask takes the box of its warped mask from the
    extents workspace and the 0.01 candidate test.  Also writes out_ref int32 (cap, 2) = (cell, object) per row and total int32 (1,) = rows
    written.  No synchronisation."""
    cp, n_cells, rp, B = _cell_table(cells, crop, k)
    cap = out_boxes.shape[0]
    assert bank_boxes.dtype == torch.float32 and bank_boxes.is_contiguous() and bank_boxes.dim() == 2 and bank_boxes.shape[1] == 4
    assert bank_labels.dtype == torch.int64 and bank_labels.is_contiguous() and offsets.dtype == torch.int64 and offsets.is_contiguous()
    assert 0 <= n_boxes <= bank_boxes.shape[0] and bank_labels.shape[0] >= n_boxes and has_mask.shape[0] >= n_boxes
    assert has_mask.dtype == torch.uint8 and has_mask.is_contiguous() and has_mask.is_cuda
    assert out_boxes.dtype == torch.float32 and out_boxes.is_contiguous() and tuple(out_boxes.shape) == (cap, 4)
    assert out_labels.dtype == torch.int64 and out_labels.is_contiguous() and tuple(out_labels.shape) == (cap,)
    assert out_img.dtype == torch.float32 and out_img.is_contiguous() and tuple(out_img.shape) == (cap,)
    assert out_ref.dtype == torch.int32 and out_ref.is_contiguous() and tuple(out_ref.shape) == (cap, 2)
    assert counts.dtype == torch.int32 and counts.is_contiguous() and overflow.dtype == torch.int32 and overflow.numel() >= 1
    assert total.dtype == torch.int32 and total.numel() >= 1
    wp, wbytes = _mask_workspace(ws, n_cells, pitch)
    _call('hdy_augment_boxes_masks', ptr(bank_boxes), ptr(bank_labels), ptr(has_mask), ptr(offsets), offsets.shape[0] - 1, int(n_boxes), cp, n_cells,
          rp, B, int(patch), int(k), int(img_size), wp, wbytes, int(pitch), ptr(out_boxes), ptr(out_labels), ptr(out_img), ptr(out_ref), cap,
          ptr(counts), counts.numel(), ptr(overflow), ptr(total))


def augment_mask_targets(instances, has_mask, offsets, n_boxes, cells, crop, patch, k, img_size, ws, pitch, out_boxes, out_ref, total, out_masks):
    """The 28 x 28 mask targets of the rows augment_boxes_masks wrote (hdy_augment_mask_targets): out_masks fp32 (cap, 28, 28); rows at or
    beyond total[0] (read on the device) are not written.  No synchronisation."""
    cp, n_cells, rp, B = _cell_table(cells, crop, k)
    ip, n, H, W = _instance_map(instances, has_mask, offsets)
    cap = out_boxes.shape[0]
    assert has_mask.shape[0] >= n_boxes >= 0
    assert out_boxes.dtype == torch.float32 and out_boxes.is_contiguous() and tuple(out_boxes.shape) == (cap, 4)
    assert out_ref.dtype == torch.int32 and out_ref.is_contiguous() and tuple(out_ref.shape) == (cap, 2)
    assert total.dtype == torch.int32 and total.numel() >= 1
    assert out_masks.dtype == torch.float32 and out_masks.is_contiguous() and tuple(out_masks.shape) == (cap, AUG_MASK_SIDE, AUG_MASK_SIDE)
    wp, wbytes = _mask_workspace(ws, n_cells, pitch)
    _call('hdy_augment_mask_targets', ip, n, H, W, ptr(has_mask), ptr(offsets), int(n_boxes), cp, n_cells, rp, B, int(patch), int(k), int(img_size),
          wp, wbytes, int(pitch), ptr(out_boxes), ptr(out_ref), ptr(total), cap, ptr(out_masks), out_masks.numel())
    return out_masks


# ------------------------------------------------------------------------------------------ detection head
def decode_level(det, anchor_px, stride, out, row_offset, level_id):
    """det: fp32 logits viewed as (B, na, ny, nx, no) with o contiguous (any other strides)."""
    require_gpu(det)
    B, na, ny, nx, no = det.shape
    assert det.dtype == torch.float32 and det.stride(4) == 1 and out.dtype == torch.float32 and out.is_contiguous()
    assert out.shape[0] == B and out.shape[2] == no + 1
    anc = (ctypes.c_float * (2 * na))(*[float(v) for v in anchor_px])
    _lib.call('hdy_decode', det.data_ptr(), det.stride(0), det.stride(1), det.stride(2), det.stride(3),
              ctypes.cast(anc, ctypes.c_void_p), float(stride), out.data_ptr(), row_offset, out.shape[1], level_id, B, na, ny, nx, no,
              stream_ptr())


def nms_batched(preds, nc, conf_thres, iou_thres, max_det, min_wh=2.0, class_aware=False):
    """preds (B, N, 5+nc+extra) fp32 on the GPU -> dict of device tensors, everything padded to max_det."""
    require_gpu(preds)
    assert preds.dtype == torch.float32 and preds.is_contiguous() and preds.dim() == 3
    B, N, row = preds.shape
    dev = preds.device
    nex = row - 5 - nc
    keep = torch.empty((B, max_det), dtype=torch.int64, device=dev)
    n_keep = torch.empty((B,), dtype=torch.int32, device=dev)
    boxes = torch.empty((B, max_det, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((B, max_det, 1 + nc), dtype=torch.float32, device=dev)
    extra = torch.empty((B, max_det, max(nex, 1)), dtype=torch.float32, device=dev)
    conf = torch.empty((B, max_det), dtype=torch.float32, device=dev)
    cls = torch.empty((B, max_det), dtype=torch.int32, device=dev)
    wsb = _lib.query('hdy_nms_workspace_bytes_for', B, N, int(max_det))
    ws = _workspace(wsb, dev)
    _lib.call('hdy_nms_batched', preds.data_ptr(), B, N, row, nc, float(conf_thres), float(iou_thres), int(max_det), float(min_wh),
              int(class_aware), keep.data_ptr(), n_keep.data_ptr(), boxes.data_ptr(), scores.data_ptr(),
              extra.data_ptr() if nex > 0 else None, conf.data_ptr(), cls.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream_ptr())
    return {'keep': keep, 'n_keep': n_keep, 'boxes': boxes, 'scores': scores, 'extra': extra[:, :, :nex], 'conf': conf, 'cls': cls}


def det_outputs(res, nc, conf_thres, pairs, multi_label=False):
    """Score / label logic of Detect.compute_outputs on nms_batched's result, compacted over the batch (hdy_det_outputs).  pairs: int32
    device tensor (npairs, 2) of (child, parent) score columns.  res['scores'] is updated in place (hierarchical products)."""
    B, max_det = res['boxes'].shape[:2]
    dev = res['boxes'].device
    C = 1 + nc
    boxes = torch.empty((B * max_det, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((B * max_det, C) if multi_label else (B * max_det,), dtype=torch.float32, device=dev)
    labels = torch.empty((B * max_det, C) if multi_label else (B * max_det,), dtype=torch.bool if multi_label else torch.int64, device=dev)
    _lib.call('hdy_det_outputs', res['scores'].data_ptr(), res['boxes'].data_ptr(), res['n_keep'].data_ptr(), B, max_det, nc,
              pairs.data_ptr() if pairs.numel() else None, pairs.shape[0], float(conf_thres), int(multi_label), boxes.data_ptr(), scores.data_ptr(),
              labels.data_ptr(), None, stream_ptr())
    return boxes, scores, labels


NMS_LDS_KEEP = 4096             # kept boxes the NMS kernel holds in LDS; calls with a larger max_det keep the list in the workspace


def _nms_launch(boxes, scores, iou_thres, max_det):
    N = boxes.shape[0]
    bs = torch.cat([boxes.float(), scores.float().reshape(N, 1)], 1).contiguous()
    keep = torch.empty((1, max_det), dtype=torch.int64, device=boxes.device)
    n_keep = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    wsb = _lib.query('hdy_nms_workspace_bytes_for', 1, N, int(max_det))
    ws = _workspace(wsb, boxes.device)
    _lib.call('hdy_nms_boxes', bs.data_ptr(), 1, N, float(iou_thres), int(max_det), keep.data_ptr(), n_keep.data_ptr(), ws.data_ptr(),
              ws.numel() * 8, stream_ptr())
    return keep[0, :int(n_keep.item())]


NMS_GRID_MIN = 32768            # nms(): sets of at least this many boxes take the multi-workgroup path (nms_grid); env HDY_NMS_GRID_MIN overrides,
#                                 0 = never.  The smallest measured size from which the new path's slowest repeat beats the one-workgroup
#                                 kernel's fastest at that and every larger measured size, over ALL three set families of
#                                 profiles/nms_grid_ab.txt; slide-like sets alone cross at 2048, tile-density sets at 8192
NMS_GRID_MAX = _lib.CONSTANTS['HDY_NMS_GRID_MAX_M']
NMS_GRID_FIRST_ROUNDS = 12      # rounds enqueued before the first look at the undecided counter (random and slide-like sets need 4-10)


def _nms_grid_min():
    v = os.environ.get('HDY_NMS_GRID_MIN')
    return NMS_GRID_MIN if v is None or v == '' else int(v)


def _nms_grid_launch(boxes, scores, iou_thres, max_det, info=None):
    """The three-piece multi-workgroup NMS (hdy_nms_grid_begin / _round / _finish) with the round loop here: rounds are enqueued in growing
    batches, and the undecided counter is read (one synchronising copy, together with the kept count) after each batch.  Returns None when the
    device flag says the spatial index cannot serve the set (a non-finite coordinate or side length): the caller falls back."""
    N = boxes.shape[0]
    dev = boxes.device
    bs = torch.cat([boxes.float(), scores.float().reshape(N, 1)], 1).contiguous()
    keep = torch.empty((max_det,), dtype=torch.int64, device=dev)
    stat = torch.empty((4,), dtype=torch.int32, device=dev)          # n_keep, then status[3] = undecided, non-finite flag, rounds
    wsb = _lib.query('hdy_nms_grid_workspace_bytes', N)
    ws = _workspace(wsb, dev)
    st = stream_ptr()
    _lib.call('hdy_nms_grid_begin', bs.data_ptr(), N, ws.data_ptr(), ws.numel() * 8, st)
    done, batch = 0, NMS_GRID_FIRST_ROUNDS
    while True:
        _lib.call('hdy_nms_grid_round', N, float(iou_thres), done, batch, ws.data_ptr(), ws.numel() * 8, st)
        done += batch
        _lib.call('hdy_nms_grid_finish', N, int(max_det), keep.data_ptr(), stat.data_ptr(), stat.data_ptr() + 4, ws.data_ptr(), ws.numel() * 8, st)
        n_keep, undecided, nonfinite, rounds = stat.tolist()
        if nonfinite:
            return None
        if undecided == 0:
            break
        batch = min(2 * batch, 1024)
    if info is not None:
        info.update(rounds=rounds, rounds_enqueued=done, workspace_bytes=wsb)
    return keep[:n_keep]


def nms_grid(boxes, scores, iou_thres, max_det=None, info=None):
    """nms() through the multi-workgroup path whatever the size: the same kept indices in the same order, bit for bit, as the one-workgroup
    kernel.  Sets the spatial index cannot serve (a non-finite coordinate, iou_thres outside [0, 1], more than NMS_GRID_MAX boxes) are
    answered by the one-workgroup kernel, as before.  `info` (a dict) receives rounds / rounds_enqueued / workspace_bytes."""
    require_gpu(boxes)
    N = boxes.shape[0]
    if N == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    max_det = N if max_det is None else max(1, min(int(max_det), N))
    iou = float(iou_thres)
    if 0.0 <= iou <= 1.0 and N <= NMS_GRID_MAX:
        keep = _nms_grid_launch(boxes, scores, iou, max_det, info)
        if keep is not None:
            return keep
    return _nms_launch(boxes, scores, iou_thres, max_det)


def nms(boxes, scores, iou_thres, max_det=None):
    """torchvision.ops.nms(boxes xyxy (N,4), scores (N,), iou) on the GPU: ALL kept indices (int64) in descending score order (ties:
    lower index first), or the first `max_det` of them, so whole-slide merges of many tiles lose nothing (the reference's torchvision call
    returns every survivor).  Below NMS_GRID_MIN boxes: one launch of the one-workgroup kernel (up to 4096 kept boxes its list lives in LDS,
    beyond that in its workspace).  From NMS_GRID_MIN on: the multi-workgroup path (nms_grid), same result bit for bit."""
    require_gpu(boxes)
    N = boxes.shape[0]
    if N == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    grid_min = _nms_grid_min()
    if grid_min > 0 and N >= grid_min:
        return nms_grid(boxes, scores, iou_thres, max_det)
    return _nms_launch(boxes, scores, iou_thres, N if max_det is None else max(1, min(int(max_det), N)))


# ------------------------------------------------------------------------------------------ detection scoring (csrc/score.hip)
AP_PRED_BLOCK, AP_TRUE_CHUNK = _lib.CONSTANTS['HDY_AP_PRED_BLOCK'], _lib.CONSTANTS['HDY_AP_TRUE_CHUNK']      # predictions per workgroup, truths per chunk
AP_MAX_IOU, AP_MAX_IGNORE = 16, 4                  # thresholds and ignored labels of one call (csrc/ap_common.h)


def _i32(t, name, who='ap_match'):
    if t is None:
        return None
    require_gpu(t)
    if t.dtype != torch.int32:
        raise _lib.HdyError(f'{who}: {name} must be int32, got {t.dtype}')
    return t.contiguous()


def _ap_rules(iouv, ignore):
    """(thresholds, their count, ignored labels, their count) as the host arrays the two matchers read"""
    thr = [float(v) for v in (iouv.tolist() if hasattr(iouv, 'tolist') else iouv)]
    ign = [int(v) for v in (ignore or ())]
    return (ctypes.c_float * max(1, len(thr)))(*thr), len(thr), (ctypes.c_longlong * max(1, len(ign)))(*ign), len(ign)


def _ap_rows(pred_scores, pred_labels, true_labels):
    """(fp32 scores, int64 prediction labels, int64 truth labels), flat and contiguous on the scores' device"""
    require_gpu(pred_scores)
    ps = pred_scores.detach().float().reshape(-1).contiguous()
    flat = lambda t: t.detach().reshape(-1).to(torch.int64).contiguous().to(ps.device)   # noqa: E731
    return ps, flat(pred_labels), flat(true_labels)


def _ap_tie_rows(who, pred_row, true_row, NP, NT):
    """the optional int32 rows of the tie rules, one entry per prediction / truth"""
    pred_row, true_row = _i32(pred_row, 'pred_row', who), _i32(true_row, 'true_row', who)
    if (pred_row is not None and pred_row.numel() != NP) or (true_row is not None and true_row.numel() != NT):
        raise _lib.HdyError(f'{who}: pred_row / true_row must have one entry per row')
    return pred_row, true_row


def _ap_outputs(NP, dev):
    """hit (16 threshold bits; torch has no unsigned 16-bit arithmetic), live, match, match_iou: one entry per prediction"""
    return tuple(torch.empty((NP,), dtype=dt, device=dev) for dt in (torch.int16, torch.uint8, torch.int32, torch.float32))


def ap_match(pred_boxes, pred_scores, pred_labels, pred_off, true_boxes, true_labels, true_off, iouv, ignore=(-100, -1), pair_iou=0.5,
             pred_row=None, true_row=None, info=None):
    """The matching of APMeter (metayolo/models/metrics.py) for a ragged batch, on the device (hdy_ap_match): image i owns prediction rows
    [pred_off[i], pred_off[i + 1]) and truth rows [true_off[i], true_off[i + 1]) (int32 device tensors of B + 1 entries).  Returns device tensors
    hit (16 bits in an int16: bit j = matched with IoU >= iouv[j]), live (uint8: 0 = touched an ignored label and unmatched), match
    (int32 truth row or -1) and match_iou (fp32), one entry per prediction row.  Equal scores inside an image rank lower row first; pred_row /
    true_row (int32) replace the position in both tie rules, so permuted inputs give the permuted results.  No host synchronisation; `info` (a
    dict) receives chunks_visited / chunks_total / workspace_bytes at the price of one read."""
    who = 'ap_match'
    require_gpu(pred_boxes)
    dev = pred_boxes.device
    pb = pred_boxes.detach().float().reshape(-1, 4).contiguous()
    tb = true_boxes.detach().float().reshape(-1, 4).contiguous()
    ps, pl, tl = _ap_rows(pred_scores, pred_labels, true_labels)
    NP, NT = pb.shape[0], tb.shape[0]
    if not (ps.numel() == NP == pl.numel() and tl.numel() == NT):
        raise _lib.HdyError(f'{who}: boxes, scores and labels disagree in length')
    pred_off, true_off = _i32(pred_off, 'pred_off'), _i32(true_off, 'true_off')
    B = pred_off.numel() - 1
    if B < 0 or true_off.numel() != B + 1:
        raise _lib.HdyError(f'{who}: pred_off and true_off must both hold B + 1 entries')
    pred_row, true_row = _ap_tie_rows(who, pred_row, true_row, NP, NT)
    wsb = _lib.query('hdy_ap_match_workspace_bytes', B, NP, NT)
    if wsb == 0:
        raise _lib.HdyError(f'{who}: counts out of range (B={B}, predictions={NP}, truths={NT})')
    out, ws = _ap_outputs(NP, dev), _workspace(wsb, dev)
    c_thr, n_thr, c_ign, n_ign = _ap_rules(iouv, ignore)
    _lib.call('hdy_ap_match', pb.data_ptr(), ps.data_ptr(), pl.data_ptr(), pred_off.data_ptr(), ptr(pred_row), NP, tb.data_ptr(), tl.data_ptr(),
              true_off.data_ptr(), ptr(true_row), NT, B, c_thr, n_thr, float(pair_iou), c_ign, n_ign, *(t.data_ptr() for t in out), ws.data_ptr(),
              _nbytes(ws), stream_ptr())
    if info is not None:
        visited, total = ws[:2].tolist()
        info.update(chunks_visited=visited, chunks_total=total, workspace_bytes=wsb)
    return out


# ------------------------------------------------------------------------------------------ mask paste (csrc/paste.hip)
PASTE_MIN_M, PASTE_MAX_M = _lib.CONSTANTS['HDY_PASTE_MIN_M'], _lib.CONSTANTS['HDY_PASTE_MAX_M']


def _paste_inputs(who, masks, boxes, padding):
    require_gpu(masks)
    require_gpu(boxes)
    if masks.dim() == 4 and masks.shape[1] == 1:
        masks = masks[:, 0]
    if masks.dim() != 3 or masks.shape[1] != masks.shape[2]:
        raise _lib.HdyError(f'{who}: masks must be (R, M, M) or (R, 1, M, M), got {tuple(masks.shape)}')
    m = masks.detach().float().contiguous()
    b = boxes.detach().float().reshape(-1, 4).contiguous()
    R, M = m.shape[0], m.shape[1]
    if b.shape[0] != R:
        raise _lib.HdyError(f'{who}: {R} masks, {b.shape[0]} boxes')
    if not PASTE_MIN_M <= M <= PASTE_MAX_M:
        raise _lib.HdyError(f'{who}: M={M} outside [{PASTE_MIN_M}, {PASTE_MAX_M}]')
    if padding not in (0, 1):
        raise _lib.HdyError(f'{who}: padding={padding} (0 or 1)')
    return m, b, R, M


def paste_masks(masks, boxes, size, padding=1):
    """torchvision's paste_masks_in_image(masks, boxes, size, padding) on the device (hdy_paste_masks; reference val_nuclei.py:169-176): masks
    (R, M, M) or (R, 1, M, M) probabilities in box coordinates, boxes (R, 4) xyxy in pixels of the (H, W) = size canvas -> (R, 1, H, W) fp32,
    the resized mask inside each (expanded, integer) box and zero elsewhere.  One launch for all rows; zero rows give an empty result."""
    m, b, R, M = _paste_inputs('paste_masks', masks, boxes, padding)
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise _lib.HdyError(f'paste_masks: canvas {H} x {W}')
    out = torch.empty((R, 1, H, W), dtype=torch.float32, device=m.device)
    if R:
        _lib.call('hdy_paste_masks', m.data_ptr(), R, M, int(padding), b.data_ptr(), out.data_ptr(), out.numel(), H, W, stream_ptr())
    return out


def paste_label_map(masks, boxes, size, window=None, threshold=0.5, padding=1, out=None):
    """One int32 label map of the (H, W) = size canvas, or of its window (x0, y0, w, h) (hdy_paste_label_map): -1 = background, otherwise the
    lowest row whose pasted mask (as paste_masks computes it) is >= threshold at the pixel — rows in descending score order, as the slide NMS
    leaves them, give every pixel to its best detection.  One launch for all rows, no host synchronisation; the map may pass 2^31 entries.
    out: a contiguous int32 (h, w) tensor to draw into (a slice of a batch of maps) instead of a new one."""
    m, b, R, M = _paste_inputs('paste_label_map', masks, boxes, padding)
    H, W = int(size[0]), int(size[1])
    x0, y0, w, h = (0, 0, W, H) if window is None else (int(v) for v in window)
    if H < 1 or W < 1 or w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise _lib.HdyError(f'paste_label_map: window {(x0, y0, w, h)} is not a non-empty part of the {H} x {W} canvas')
    if out is None:
        out = torch.empty((h, w), dtype=torch.int32, device=m.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (h, w) or not out.is_contiguous() or out.device != m.device:
        raise _lib.HdyError(f'paste_label_map: out must be a contiguous int32 ({h}, {w}) tensor on {m.device}')
    _lib.call('hdy_paste_label_map', ptr(m) if R else None, R, M, int(padding), ptr(b) if R else None, float(threshold), x0, y0, out.data_ptr(),
              out.numel(), h, w, stream_ptr())
    return out


def label_areas(label_map, R):
    """areas (int32, R entries): pixels of the int32 label map that each row owns (hdy_label_areas)"""
    require_gpu(label_map)
    if label_map.dtype != torch.int32:
        raise _lib.HdyError(f'label_areas: the map must be int32, got {label_map.dtype}')
    lm = label_map.contiguous()
    R = int(R)
    areas = torch.empty((R,), dtype=torch.int32, device=lm.device)
    if R:
        _lib.call('hdy_label_areas', ptr(lm) if lm.numel() else None, lm.numel(), areas.data_ptr(), R, stream_ptr())
    return areas


# ------------------------------------------------------------------------------------------ label measurement (csrc/measure.hip)
def _label_inputs(who, label_map, R, extent=None):
    """(the map contiguous, R, the extent contiguous) of a non-empty int32 (h, w) label map on the GPU, a row count and, where the pass reads
    one, the int32 (R, 4) extent table on the map's device"""
    require_gpu(label_map)
    if label_map.dtype != torch.int32 or label_map.dim() != 2 or label_map.numel() == 0:
        raise _lib.HdyError(f'{who}: the map must be a non-empty int32 (h, w) tensor, got {label_map.dtype} {tuple(label_map.shape)}')
    R = int(R)
    if R < 0:
        raise _lib.HdyError(f'{who}: negative row count R={R}')
    lm = label_map.contiguous()
    if extent is not None:
        require_gpu(extent)
        if extent.dtype != torch.int32 or tuple(extent.shape) != (R, 4) or extent.device != lm.device:
            raise _lib.HdyError(f'{who}: extent must be an int32 ({R}, 4) tensor on {lm.device} (ops.label_measure makes it), got '
                                f'{extent.dtype} {tuple(extent.shape)} on {extent.device}')
        extent = extent.contiguous()
    return lm, R, extent


def _image_window(who, image, lm, window):
    """(ip, nbytes, pitch, pb, x0, y0) as the label passes take the 8-bit image under the map: the view slide_u8 accepts, on the map's device,
    of which the map covers the window at (x0, y0) = window; image None gives a null pointer and zeros"""
    x0, y0 = (int(v) for v in window)
    if image is None:
        return None, 0, 0, 0, x0, y0
    h, w = lm.shape
    ip, pitch, pb, H, W = slide_u8(image)
    if image.device != lm.device:
        raise _lib.HdyError(f'{who}: the map is on {lm.device}, the image on {image.device}')
    if x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise _lib.HdyError(f'{who}: the {h} x {w} map at window origin {(x0, y0)} leaves the {H} x {W} image')
    return ip, (H - 1) * pitch + W * pb, pitch, pb, x0, y0        # nbytes: from the first byte of the view to the last byte of its last pixel


def label_measure(label_map, R, image=None, window=(0, 0), origin=None):
    """(sums, extent) of the R labels of an int32 (h, w) label map (hdy_label_measure, include/hdyolo_measure.h): sums int64 (R, 14) = n, sum dx,
    sum dy, sum dx^2, sum dy^2, sum dx dy, boundary edges, edges on the window border, sum R, G, B, sum R^2, G^2, B^2 with dx = j - ox, dy = i - oy;
    extent int32 (R, 4) = min j, min i, max j, max i ({w, h, -1, -1} for a label that owns nothing).  One pass, integer-exact, no synchronisation.
    image: the 8-bit slide as slide_u8 takes it ((H, W, 3 | 4) uint8, any row stride), of which the map covers the window at (x0, y0) = window;
    None leaves the stain columns zero.  origin: int32 (R, 2) = (ox, oy) per label in map coordinates (None = zeros); hd_yolo_amd/measure.py
    (nucleus_table) turns the sums into the measurements."""
    lm, R, _ = _label_inputs('label_measure', label_map, R)
    h, w = lm.shape
    window = _image_window('label_measure', image, lm, window)
    if origin is not None:
        require_gpu(origin)
        if origin.dtype != torch.int32 or tuple(origin.shape) != (R, 2) or origin.device != lm.device:
            raise _lib.HdyError(f'label_measure: origin must be an int32 ({R}, 2) tensor on {lm.device}, got {origin.dtype} {tuple(origin.shape)}')
        origin = origin.contiguous()
    sums = torch.empty((R, _ext.CONSTANTS['HDY_MEASURE_COLS']), dtype=torch.int64, device=lm.device)
    extent = torch.empty((R, 4), dtype=torch.int32, device=lm.device)
    if R:
        _ext.call('hdy_label_measure', lm.data_ptr(), lm.numel(), h, w, *window, ptr(origin), sums.data_ptr(), sums.numel(),
                  extent.data_ptr(), extent.numel(), R, stream_ptr())
    return sums, extent


# ------------------------------------------------------------------------------------------ outlines and hulls (csrc/outline.hip)
def label_outline(label_map, R, extent):
    """(offsets int64 (R + 1,), verts int32 (total, 2), counts int64 (R, 4)) of the R labels of an int32 (h, w) label map: the outer boundary
    of every label's first 4-connected component as a closed polygon of lattice corners (x, y), clockwise on screen, the start corner first
    (include/hdyolo_outline.h states the geometry).  extent: the int32 (R, 4) boxes of ops.label_measure on the same map.  counts = {V, twice
    the enclosed area, unit cracks L, flags (1 empty, 2 box side above 1024, 4 the extent was not this map's)}; the vertices of label r are
    verts[offsets[r]:offsets[r + 1]].  Two launches (hdy_label_outline_count, hdy_label_outline_write) with torch.cumsum between them on the
    device.  `total`, the number of vertices, is the one scalar of the result this call reads back: it sizes verts.  The status word of the
    writing pass (non-zero when the second walk disagrees with the first) is read once the pass is queued and raises."""
    lm, R, extent = _label_inputs('label_outline', label_map, R, extent)
    h, w = lm.shape
    dev = lm.device
    counts = torch.empty((R, 4), dtype=torch.int64, device=dev)
    offsets = torch.zeros((R + 1,), dtype=torch.int64, device=dev)
    if R == 0:
        return offsets, torch.empty((0, 2), dtype=torch.int32, device=dev), counts
    head = (lm.data_ptr(), lm.numel(), h, w, extent.data_ptr(), extent.numel(), R)
    _ext.call('hdy_label_outline_count', *head, counts.data_ptr(), counts.numel(), stream_ptr())
    torch.cumsum(counts[:, 0], 0, out=offsets[1:])
    total = int(offsets[-1])                                              # the read-back that sizes verts
    verts = torch.empty((total, 2), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    _ext.call('hdy_label_outline_write', *head, offsets.data_ptr(), offsets.numel(), verts.data_ptr() if total else None, verts.numel(),
              status.data_ptr(), stream_ptr())
    if int(status):
        raise _lib.HdyError('label_outline: the writing pass counted other vertices than the counting pass (status 1): the map or the extent '
                            'changed between the two launches')
    return offsets, verts, counts


def label_hull(label_map, R, extent):
    """(hull_i int64 (R, 4), hull_f float64 (R, 2)) of the R labels of an int32 (h, w) label map (hdy_label_hull, include/hdyolo_outline.h): the
    convex hull of all pixel squares of every label, fragments included, holes ignored.  hull_i = {hull vertices, twice the hull area, squared
    maximum Feret diameter, flags as label_outline's}, exact; hull_f = {hull perimeter, minimum Feret diameter}.  extent: ops.label_measure's.
    One pass, nothing is read back."""
    lm, R, extent = _label_inputs('label_hull', label_map, R, extent)
    h, w = lm.shape
    hull_i = torch.empty((R, 4), dtype=torch.int64, device=lm.device)
    hull_f = torch.empty((R, 2), dtype=torch.float64, device=lm.device)
    if R:
        _ext.call('hdy_label_hull', lm.data_ptr(), lm.numel(), h, w, extent.data_ptr(), extent.numel(), R, hull_i.data_ptr(), hull_i.numel(),
                  hull_f.data_ptr(), hull_f.numel(), stream_ptr())
    return hull_i, hull_f


# ------------------------------------------------------------------------------------------ texture counts (csrc/texture.hip)
def label_texture(label_map, R, extent, image, lut, levels=16, offsets=TEXTURE_OFFSETS, window=(0, 0), rows=None):
    """(hist int32 (n, levels), glcm int32 (n, D, levels, levels), flags int32 (n,)) of the labels row0 .. row0 + n - 1 of an int32 (h, w) label
    map (hdy_label_texture, include/hdyolo_texture.h); rows = (row0, n), None = all R.  Per label, over its entries inside its box: the
    histogram of the pixels' levels and, per offset (di, dj), the symmetric co-occurrence matrix of the levels of the pairs of entries of the
    label that lie that far apart.  extent: the int32 (R, 4) boxes of ops.label_measure on the same map.  image: the 8-bit slide as slide_u8
    takes it, of which the map covers the window at (x0, y0) = window.  lut: int32 (3, 256), level = clamp((lut[0][R] + lut[1][G] + lut[2][B])
    >> 16, 0, levels - 1) (hd_yolo_amd/texture.py: stain_lut); levels 8, 16 or 32; at most 4 offsets of reach 4.  flags: 0 measured, 1 the
    label owns nothing, 2 a box side above 1024 (zeros).  One pass, integer-exact, nothing is read back."""
    who = 'label_texture'
    lm, R, extent = _label_inputs(who, label_map, R, extent)
    h, w = lm.shape
    dev = lm.device
    if image is None:
        raise _lib.HdyError(f'{who}: the pass needs the 8-bit image under the map')
    window = _image_window(who, image, lm, window)
    require_gpu(lut)
    if lut.dtype != torch.int32 or tuple(lut.shape) != (3, 256) or lut.device != dev:
        raise _lib.HdyError(f'{who}: lut must be an int32 (3, 256) tensor on {dev}, got {lut.dtype} {tuple(lut.shape)} on {lut.device}')
    lut = lut.contiguous()
    levels = int(levels)
    if levels not in (8, 16, 32):
        raise _lib.HdyError(f'{who}: levels={levels} (8, 16 or 32)')
    offs = [(int(di), int(dj)) for di, dj in offsets]
    D = len(offs)
    if not 1 <= D <= _ext.CONSTANTS['HDY_TEXTURE_MAX_OFFSETS']:
        raise _lib.HdyError(f'{who}: {D} offsets (1 to {_ext.CONSTANTS["HDY_TEXTURE_MAX_OFFSETS"]})')
    row0, n = (0, R) if rows is None else (int(v) for v in rows)
    if row0 < 0 or n < 0 or row0 + n > R:
        raise _lib.HdyError(f'{who}: rows=({row0}, {n}) outside the {R} labels')
    hist = torch.empty((n, levels), dtype=torch.int32, device=dev)
    glcm = torch.empty((n, D, levels, levels), dtype=torch.int32, device=dev)
    flags = torch.empty((n,), dtype=torch.int32, device=dev)
    host_offsets = (ctypes.c_int * (2 * D))(*(v for o in offs for v in o))        # a host array: the entry point reads it before it returns
    if n:
        _ext.call('hdy_label_texture', lm.data_ptr(), lm.numel(), h, w, *window, extent.data_ptr(), extent.numel(), R,
                  lut.data_ptr(), lut.numel(), levels, host_offsets, 2 * D, D, row0, n, hist.data_ptr(), hist.numel(), glcm.data_ptr(),
                  glcm.numel(), flags.data_ptr(), flags.numel(), stream_ptr())
    return hist, glcm, flags


# ------------------------------------------------------------------------------------------ neighbourhood features (csrc/spatial.hip)
def _spatial_inputs(who, xy_units, cls, C):
    """(xy int32 (N, 2) contiguous, class int32 (N,) with every class outside [0, C) as -1) of a point set on the GPU"""
    require_gpu(xy_units)
    if xy_units.dtype != torch.int32 or xy_units.dim() != 2 or xy_units.shape[1] != 2:
        raise _lib.HdyError(f'{who}: positions must be an int32 (N, 2) tensor of units, got {xy_units.dtype} {tuple(xy_units.shape)}')
    N = xy_units.shape[0]
    if cls.dtype not in (torch.int32, torch.int64) or tuple(cls.shape) != (N,) or cls.device != xy_units.device:
        raise _lib.HdyError(f'{who}: classes must be an int32 / int64 ({N},) tensor on {xy_units.device}, got {cls.dtype} {tuple(cls.shape)} on '
                            f'{cls.device}')
    C = int(C)
    return xy_units.contiguous(), torch.where((cls >= 0) & (cls < C), cls, -1).to(torch.int32), N, C


def _spatial_pts(xy, cls32, order=None):
    """pts int32 (N, 4) = (x, y, class, original row), in `order` when given"""
    rows = torch.arange(xy.shape[0], dtype=torch.int32, device=xy.device)
    pts = torch.stack([xy[:, 0], xy[:, 1], cls32, rows], 1)
    return (pts if order is None else pts[order]).contiguous()


def _sorted_points(who, pts, cell_start=None):
    """check points in cell order (contiguous int32 (N, 4) on the GPU) and, when given, their cell_start"""
    require_gpu(pts)
    if cell_start is not None:
        require_gpu(cell_start)
    if pts.dtype != torch.int32 or pts.dim() != 2 or pts.shape[1] != 4 or not pts.is_contiguous():
        raise _lib.HdyError(f'{who}: pts must be a contiguous int32 (N, 4) tensor, got {pts.dtype} {tuple(pts.shape)}')
    if cell_start is not None and (cell_start.dtype != torch.int32 or cell_start.dim() != 1 or not cell_start.is_contiguous()
                                   or cell_start.device != pts.device):
        raise _lib.HdyError(f'{who}: cell_start must be a contiguous int32 vector on {pts.device}, got {cell_start.dtype} '
                            f'{tuple(cell_start.shape)}')


def spatial_cells(pts, cell_units, ncx, ncy):
    """(cell_start int32 (ncx * ncy + 1,), status int32 (1,)) of points in cell order (hdy_spatial_cells, include/hdyolo_spatial.h): pts int32
    (N, 4) = (x, y, class, original row) sorted by cell, absent points last.  status is a device word, non-zero when pts is not in cell order;
    nothing is read back."""
    _sorted_points('spatial_cells', pts)
    ncx, ncy = int(ncx), int(ncy)
    cell_start = torch.empty((max(ncx * ncy, 0) + 1,), dtype=torch.int32, device=pts.device)
    status = torch.empty((1,), dtype=torch.int32, device=pts.device)
    N = pts.shape[0]
    _ext.call('hdy_spatial_cells', pts.data_ptr() if N else None, pts.numel(), N, int(cell_units), ncx, ncy, cell_start.data_ptr(), cell_start.numel(),
              status.data_ptr(), 1, stream_ptr())
    if N == 0:
        cell_start.zero_()
        status.zero_()
    return cell_start, status


def spatial_neighbors_sorted(pts, cell_start, cell_units, ncx, ncy, radii_units, C):
    """(counts int32 (N, K, C), near_d2 int64 (N, C), near_row int32 (N, C)) from points in cell order and their cell_start
    (hdy_spatial_neighbors): the second half of spatial_neighbors, rows of the outputs = the points' original rows."""
    _sorted_points('spatial_neighbors', pts, cell_start)
    radii = [int(r) for r in radii_units]
    N, K, C = pts.shape[0], len(radii), int(C)
    dev = pts.device
    counts = torch.empty((N, K, max(C, 0)), dtype=torch.int32, device=dev)
    near_d2 = torch.empty((N, max(C, 0)), dtype=torch.int64, device=dev)
    near_row = torch.empty((N, max(C, 0)), dtype=torch.int32, device=dev)
    host_radii = (ctypes.c_int * max(K, 1))(*radii)                       # a host array: the entry point reads it before it returns
    p = (lambda t: t.data_ptr() if N else None)
    _ext.call('hdy_spatial_neighbors', p(pts), pts.numel(), N, cell_start.data_ptr(), cell_start.numel(), int(cell_units), int(ncx), int(ncy),
              host_radii, K, C, p(counts), counts.numel(), p(near_d2), near_d2.numel(), p(near_row), near_row.numel(), stream_ptr())
    return counts, near_d2, near_row


SPATIAL_GRID_SIDE = 4096        # spatial_neighbors: at most this many cells along a side, whatever the extent (score_slide's bound)


def _cell_index(who, xy, cls32, N, cell_units, default_cell, extent_units, info):
    """(pts, cell_start, cell, ncx, ncy), the leading arguments of the *_sorted calls: the first half of spatial_neighbors and spatial_knn, whose
    docstrings state it.  default_cell(mx, my): the cell side when cell_units is None, from the largest coordinates the grid covers."""
    present = (xy >= 0).all(1)
    if extent_units is None:
        mx, my = torch.where(present[:, None], xy, 0).amax(0).tolist() if N else (0, 0)
    else:
        mx, my = (max(int(v) - 1, 0) for v in extent_units)
    cell = default_cell(mx, my) if cell_units is None else int(cell_units)
    if cell < 1:
        raise _lib.HdyError(f'{who}: cell_units={cell} must be positive')
    ncx, ncy = mx // cell + 1, my // cell + 1
    cx = torch.div(xy[:, 0], cell, rounding_mode='floor').clamp(max=ncx - 1)
    cy = torch.div(xy[:, 1], cell, rounding_mode='floor').clamp(max=ncy - 1)
    cid = torch.where(present, cy.to(torch.int64) * ncx + cx, ncx * ncy)          # absent points behind every cell
    pts = _spatial_pts(xy, cls32, torch.sort(cid, stable=True)[1])
    cell_start, status = spatial_cells(pts, cell, ncx, ncy)
    if info is not None:
        info.update(status=status, cell_units=cell, ncx=ncx, ncy=ncy, pts=pts, cell_start=cell_start)
    return pts, cell_start, cell, ncx, ncy


def spatial_neighbors(xy_units, cls, C, radii_units, cell_units=None, extent_units=None, info=None):
    """(counts, near_d2, near_row) of a point set (include/hdyolo_spatial.h): per point, the number of other points of every class c in [0, C)
    within each of the K radii (counts int32 (N, K, C), cumulative), the squared distance in units to the nearest one of every class within
    the largest radius (near_d2 int64 (N, C), -1 = none) and its row (near_row int32 (N, C), lowest row among equals, -1 = none).
    xy_units int32 (N, 2) in units of 1/16 pixel (hd_yolo_amd/spatial.py: to_units); a negative coordinate makes the point absent.  cls: int32 /
    int64 (N,); a class outside [0, C) makes the point a query only.  radii_units: K strictly increasing integers.
    cell_units: the side of a search cell (default max(r_K, ceil(extent / 4096))); the result does not depend on it.  extent_units = (x, y)
    bounds of the coordinates when the caller knows them (the slide's size): without it the largest coordinates are read back once, to size
    the grid.  The points are ordered by cell with one stable device sort, packed, and handed to hdy_spatial_cells and hdy_spatial_neighbors.
    info (a dict) receives 'status' (the device word of hdy_spatial_cells: 0 unless the order was broken), 'cell_units', 'ncx', 'ncy' and the
    workspace of the two calls, 'pts' (the packed points in cell order) and 'cell_start'."""
    xy, cls32, N, C = _spatial_inputs('spatial_neighbors', xy_units, cls, C)
    radii = [int(r) for r in radii_units]
    if not radii:
        raise _lib.HdyError('spatial_neighbors: no radii')
    default_cell = (lambda mx, my: max(radii[-1], -(-(max(mx, my) + 1) // SPATIAL_GRID_SIDE), 1))
    return spatial_neighbors_sorted(*_cell_index('spatial_neighbors', xy, cls32, N, cell_units, default_cell, extent_units, info), radii, C)


def spatial_density(xy_units, cls, C, g_units, gx, gy):
    """grid int32 (gy, gx, C): the present points of class c in [0, C) whose position falls into field (y // g_units, x // g_units)
    (hdy_spatial_density); points outside the gx x gy fields, absent points and query-only points are not counted.  Integer adds only."""
    xy, cls32, N, C = _spatial_inputs('spatial_density', xy_units, cls, C)
    gx, gy = int(gx), int(gy)
    pts = _spatial_pts(xy, cls32)
    grid = torch.empty((max(gy, 0), max(gx, 0), max(C, 0)), dtype=torch.int32, device=xy.device)
    _ext.call('hdy_spatial_density', pts.data_ptr() if N else None, pts.numel(), N, int(g_units), gx, gy, C, grid.data_ptr() if grid.numel() else None,
              grid.numel(), stream_ptr())
    if N == 0:
        grid.zero_()                                                      # N = 0 launches nothing
    return grid


# ------------------------------------------------------------------------------------------ k nearest neighbours (csrc/graph.hip)
KNN_CELL_FILL = 0.25            # spatial_knn's default cell aims at this many times k points per cell: a lane then searches two rings or three, about 6 k
                                # candidates; 2, 1 and 0.5 each lost the sweep of scripts/bench_graph.py to its half


def spatial_knn_sorted(pts, cell_start, cell_units, ncx, ncy, k, max_radius_units):
    """(nbr_row int32 (N, k), nbr_d2 int64 (N, k), nbr_count int32 (N,)) from points in cell order and their cell_start (hdy_graph_knn,
    include/hdyolo_graph.h): the second half of spatial_knn, rows of the outputs = the points' original rows."""
    _sorted_points('spatial_knn', pts, cell_start)
    N, k = pts.shape[0], int(k)
    dev = pts.device
    nbr_row = torch.empty((N, max(k, 0)), dtype=torch.int32, device=dev)
    nbr_d2 = torch.empty((N, max(k, 0)), dtype=torch.int64, device=dev)
    nbr_count = torch.empty((N,), dtype=torch.int32, device=dev)
    p = (lambda t: t.data_ptr() if N else None)
    _ext.call('hdy_graph_knn', p(pts), pts.numel(), N, cell_start.data_ptr(), cell_start.numel(), int(cell_units), int(ncx), int(ncy), k,
              int(max_radius_units), p(nbr_row), nbr_row.numel(), p(nbr_d2), nbr_d2.numel(), p(nbr_count), nbr_count.numel(), stream_ptr())
    return nbr_row, nbr_d2, nbr_count


def knn_cell_units(N, k, max_radius_units, mx, my, fill=KNN_CELL_FILL):
    """The default cell side of spatial_knn, host arithmetic only: the side at which a cell of an (mx + 1) x (my + 1) extent with N points
    spread evenly holds fill * k of them, floored by ceil(max_radius / HDY_GRAPH_MAX_RINGS) (the ring bound of hdy_graph_knn) and by
    ceil(extent / SPATIAL_GRID_SIDE)."""
    import math
    want = math.isqrt(int((mx + 1) * (my + 1) * fill * max(int(k), 1)) // max(int(N), 1))
    return max(want, -(-int(max_radius_units) // _ext.CONSTANTS['HDY_GRAPH_MAX_RINGS']), -(-(max(mx, my) + 1) // SPATIAL_GRID_SIDE), 1)


def spatial_knn(xy_units, k, max_radius_units, cls=None, C=None, cell_units=None, extent_units=None, info=None):
    """(nbr_row, nbr_d2, nbr_count) of a point set (include/hdyolo_graph.h): per point the rows of its k nearest other nodes within
    max_radius_units, nearest first, ties by the lowest row (nbr_row int32 (N, k), -1 padding), their squared distances in units (nbr_d2 int64
    (N, k), -1 padding) and how many there are (nbr_count int32 (N,)).
    xy_units int32 (N, 2) in units of 1/16 pixel; a negative coordinate makes the point absent (-1 / -1 / 0).  With cls (int32 / int64 (N,)) and C,
    a point of a class outside [0, C) is a query only: it gets neighbours and is nobody's; without them every present point is a node.
    cell_units: the side of a search cell (default knn_cell_units: about KNN_CELL_FILL * k points per cell); the result does not depend on it,
    but ceil(max_radius_units / cell_units) may not pass HDY_GRAPH_MAX_RINGS.  extent_units = (x, y) bounds of the coordinates when the caller
    knows them: without it the largest coordinates are read back once, to size the grid; with it nothing is read back.  The points are ordered
    by cell with one stable device sort, packed, and handed to hdy_spatial_cells and hdy_graph_knn.  info (a dict) receives what
    spatial_neighbors puts there: 'status', 'cell_units', 'ncx', 'ncy', 'pts' and 'cell_start'."""
    if (cls is None) != (C is None):
        raise _lib.HdyError('spatial_knn: cls and C go together')
    if cls is None:
        require_gpu(xy_units)
        cls, C = torch.zeros((xy_units.shape[0] if xy_units.dim() else 0,), dtype=torch.int32, device=xy_units.device), 1
    xy, cls32, N, C = _spatial_inputs('spatial_knn', xy_units, cls, C)
    k, rmax = int(k), int(max_radius_units)
    default_cell = (lambda mx, my: knn_cell_units(N, k, rmax, mx, my))
    return spatial_knn_sorted(*_cell_index('spatial_knn', xy, cls32, N, cell_units, default_cell, extent_units, info), k, rmax)


def knn_mutual(nbr_row):
    """mutual int32 (N, k) of nbr_row int32 (N, k) (hdy_graph_mutual): entry (p, s) is 1 when q = nbr_row[p, s] is a row and p is among q's
    neighbours, else 0.  Any content of nbr_row is safe."""
    require_gpu(nbr_row)
    if nbr_row.dtype != torch.int32 or nbr_row.dim() != 2:
        raise _lib.HdyError(f'knn_mutual: nbr_row must be an int32 (N, k) tensor, got {nbr_row.dtype} {tuple(nbr_row.shape)}')
    nbr_row = nbr_row.contiguous()
    N, k = nbr_row.shape
    mutual = torch.empty((N, k), dtype=torch.int32, device=nbr_row.device)
    p = (lambda t: t.data_ptr() if N else None)
    _ext.call('hdy_graph_mutual', p(nbr_row), nbr_row.numel(), N, k, p(mutual), mutual.numel(), stream_ptr())
    return mutual


# ------------------------------------------------------------------------------------------ mask scoring (csrc/mask_score.hip)
OVERLAP_MIN_SLOTS, OVERLAP_MAX_SLOTS = 64, _lib.CONSTANTS['HDY_OVERLAP_MAX_SLOTS']


def _pow2_at_least(n, lo=OVERLAP_MIN_SLOTS):
    s = lo
    while s < n:
        s <<= 1
    return s


def _label_map_i32(who, t, name, rows):
    """an int32 label map as it is; the tile bank's 16-bit instance map (uint16, or the same bits as int16) widened, 0xFFFF staying 65535:
    background only while the `rows` it is scored against (all segments together) do not pass 65535, so more rows are refused"""
    require_gpu(t)
    if t.dtype == torch.int32:
        return t.contiguous()
    if t.dtype in (torch.uint16, torch.int16) and rows > 0xFFFF:
        raise _lib.HdyError(f'{who}: a 16-bit {name} marks background with 0xFFFF, which is a row once there are {rows} > 65535 of them: pass an '
                            f'int32 map with negative background')
    if t.dtype == torch.uint16:
        return t.contiguous().view(torch.int16).to(torch.int32).bitwise_and_(0xFFFF)
    if t.dtype == torch.int16:
        return t.to(torch.int32).bitwise_and_(0xFFFF)
    raise _lib.HdyError(f'{who}: {name} must be int32 or a 16-bit instance map, got {t.dtype}')


def _overlap_table(slots, dev):
    """keys uint64 [slots] | counts uint32 [slots] in one buffer (include/hdyolo.h): the buffer and its two views"""
    buf = torch.empty((slots * 3 // 2,), dtype=torch.int64, device=dev)
    return buf, buf[:slots], buf[slots:].view(torch.int32)


def label_overlap(pred_map, true_map, n_pred, n_true, seg=None, max_pairs=None):
    """The overlap of two label maps of equal shape as a sparse contingency table (hdy_label_overlap): returns (pairs, pred_area, true_area),
    pairs an (n, 3) int64 device tensor of (p, t, shared entries > 0) sorted by (p, t), the areas int32 entry counts per row.  pred_map int32
    (-1 background, as paste_label_map leaves it), true_map int32 or the tile bank's uint16 instance map; a label that is negative or not below
    n_pred / n_true is background.  seg = (pred_base, true_base), int32 device tensors of n_seg entries: the maps are n_seg equal segments along
    their first dimension (a batch of tile maps) and segment s's non-negative labels are shifted by the bases, so tile-local rows become rows of
    the concatenated arrays.  max_pairs sizes the table (default: from n_pred + n_true; a power of two of at least twice the pairs is taken).
    One read (the status pair), after which the table is compacted and sorted on the device; HdyError when the table was too small."""
    who = 'label_overlap'
    n_pred, n_true = int(n_pred), int(n_true)
    if n_pred < 0 or n_true < 0:
        raise _lib.HdyError(f'{who}: negative row count')
    pm, tm = _label_map_i32(who, pred_map, 'pred_map', n_pred), _label_map_i32(who, true_map, 'true_map', n_true)
    if pm.shape != tm.shape:
        raise _lib.HdyError(f'{who}: the maps disagree in shape: {tuple(pm.shape)} and {tuple(tm.shape)}')
    dev = pm.device
    n_seg, seg_elems, pbase, tbase = 0, 0, None, None
    if seg is not None:
        pbase, tbase = _i32(seg[0], 'pred_base', who), _i32(seg[1], 'true_base', who)
        n_seg = pbase.numel()
        if n_seg < 1 or tbase.numel() != n_seg or pm.dim() < 1 or pm.shape[0] != n_seg:
            raise _lib.HdyError(f'{who}: seg bases must both hold one entry per segment (the first dimension of the maps)')
        seg_elems = pm.numel() // n_seg
    slots = _pow2_at_least(2 * int(max_pairs) if max_pairs is not None else 4 * (n_pred + n_true), 8 if max_pairs is not None else OVERLAP_MIN_SLOTS)
    if slots > OVERLAP_MAX_SLOTS:
        raise _lib.HdyError(f'{who}: a table of {slots} slots passes {OVERLAP_MAX_SLOTS}')
    buf, keys, counts = _overlap_table(slots, dev)
    parea = torch.empty((n_pred,), dtype=torch.int32, device=dev)
    tarea = torch.empty((n_true,), dtype=torch.int32, device=dev)
    status = torch.empty((2,), dtype=torch.int32, device=dev)
    _lib.call('hdy_label_overlap', ptr(pm) if pm.numel() else None, ptr(tm) if tm.numel() else None, pm.numel(), seg_elems, n_seg, ptr(pbase),
              ptr(tbase), n_pred, n_true, ptr(parea) if n_pred else None, ptr(tarea) if n_true else None, buf.data_ptr(), _nbytes(buf), slots,
              status.data_ptr(), stream_ptr())
    n, overflow = status.tolist()                                   # the one read
    if overflow:
        raise _lib.HdyError(f'{who}: the pair table of {slots} slots is full ({overflow} inserts failed): pass a larger max_pairs')
    skeys, order = torch.sort(keys)                                 # unused slots hold -1 and sort first
    skeys, cnt = skeys[slots - n:], counts[order[slots - n:]]
    pairs = torch.stack([skeys >> 32, skeys & 0xFFFFFFFF, cnt.to(torch.int64)], 1)
    return pairs, parea, tarea


def mask_ap_match(pairs, pred_area, true_area, pred_scores, pred_labels, true_labels, iouv, ignore=(-100, -1), pair_iou=0.5, pred_row=None,
                  true_row=None):
    """ops.ap_match with the IoU of instance masks (hdy_mask_ap_match): pairs / pred_area / true_area as label_overlap returns them, scores,
    labels and the optional pred_row / true_row one per row of the concatenated arrays (rows of different images never share a pair, so there
    are no offsets).  IoU = float(inter) / float(area_p + area_t - inter).  Returns hit (16 threshold bits in an int16), live (uint8), match
    (int32 truth row or -1) and match_iou (fp32), one entry per prediction.  No host synchronisation."""
    who = 'mask_ap_match'
    ps, pl, tl = _ap_rows(pred_scores, pred_labels, true_labels)
    dev, NP, NT = ps.device, ps.numel(), tl.numel()
    pa, ta = _i32(pred_area, 'pred_area', who), _i32(true_area, 'true_area', who)
    if not (pl.numel() == NP == pa.numel() and ta.numel() == NT):
        raise _lib.HdyError(f'{who}: scores, labels and areas disagree in length')
    pred_row, true_row = _ap_tie_rows(who, pred_row, true_row, NP, NT)
    require_gpu(pairs)
    if pairs.dim() != 2 or pairs.shape[1] != 3 or pairs.dtype != torch.int64:
        raise _lib.HdyError(f'{who}: pairs must be an (n, 3) int64 tensor, got {pairs.dtype} {tuple(pairs.shape)}')
    n = pairs.shape[0]
    slots = _pow2_at_least(n)
    buf, keys, counts = _overlap_table(slots, dev)                  # the kernel walks every slot, so the compacted pairs are a table as they are
    keys[:n] = (pairs[:, 0] << 32) | pairs[:, 1]
    keys[n:] = -1
    counts[:n] = pairs[:, 2].to(torch.int32)
    counts[n:] = 0
    out, ws = _ap_outputs(NP, dev), _workspace(_lib.query('hdy_mask_ap_match_workspace_bytes', NP, NT), dev)
    p = lambda t: ptr(t) if t.numel() else None                     # noqa: E731  (no rows: a null pointer)
    c_thr, n_thr, c_ign, n_ign = _ap_rules(iouv, ignore)
    _lib.call('hdy_mask_ap_match', buf.data_ptr(), _nbytes(buf), slots, p(pa), p(ta), p(ps), p(pl), ptr(pred_row), NP, p(tl), ptr(true_row), NT, c_thr,
              n_thr, float(pair_iou), c_ign, n_ign, *(p(t) for t in out), ws.data_ptr(), _nbytes(ws), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------ mask branch primitives (row f2)
def roi_align(feat, rois, spatial_scale, P, sampling_ratio=2, aligned=False):
    """feat NHWC (B, H, W, C) (possibly a pitched view), rois (R, 5) fp32 [image, x1, y1, x2, y2] -> (R, P, P, C) NHWC."""
    fp, B, H, W, C, ldf = nhwc(feat)
    R = rois.shape[0]
    out = torch.empty((R, P, P, C), dtype=feat.dtype, device=feat.device)
    rois = rois.float().contiguous()
    _lib.call('hdy_roi_align_fwd', fp, ldf, B, H, W, C, rois.data_ptr(), R, float(spatial_scale), P, sampling_ratio, int(aligned),
              out.data_ptr(), dcode(feat.dtype), stream_ptr())
    return out


_RoiLevel = _lib.RoiLevel
ROI_LEVELS_MAX, ROI_LEVELS_MAX_B = 8, 1024           # hdy_roi_align_levels_fwd (include/hdyolo.h)


def roi_align_levels(feats, scales, res, out_rows, P, sampling_ratio=2, aligned=False, out=None):
    """Multi-level roi_align over a batch's detections in one launch (hdy_roi_align_levels_fwd).  feats: per level an NHWC (B, H, W, C) map
    (possibly a pitched view; one C and dtype), scales: per level spatial_scale; res: nms_batched's result — padded boxes (B, max_det, 4), the
    level id as column 0 of 'extra', the device n_keep.  -> (out_rows, P, P, C) NHWC in compacted order (image b's rows at
    n_keep[0] + .. + n_keep[b - 1]); out_rows is a host value, normally sum(n_keep); rows behind the device total are left unwritten.
    out: a contiguous (out_rows, P, P, C) tensor of the maps' dtype to write into instead of a new one."""
    boxes, extra, n_keep = res['boxes'], res['extra'], res['n_keep']
    require_gpu(boxes)
    nl = len(feats)
    assert nl == len(scales) and 1 <= nl <= ROI_LEVELS_MAX, f'{nl} levels, {len(scales)} scales (1 .. {ROI_LEVELS_MAX} levels)'
    B, max_det = boxes.shape[:2]
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.shape[2] == 4
    assert extra.dtype == torch.float32 and extra.dim() == 3 and tuple(extra.shape[:2]) == (B, max_det) and extra.shape[2] >= 1 \
        and extra.stride(2) == 1 and extra.stride(0) == max_det * extra.stride(1), f'level column of the NMS result: {extra.shape} {extra.stride()}'
    assert n_keep.dtype == torch.int32 and n_keep.is_contiguous() and n_keep.numel() == B and 1 <= B <= ROI_LEVELS_MAX_B
    dtype, C = feats[0].dtype, feats[0].shape[3]
    table = (_RoiLevel * nl)()
    for l, f in enumerate(feats):
        fp, n, h, w, c, ldf = nhwc(f)
        assert f.dtype == dtype and c == C and n >= B and f.device == boxes.device, f'level {l}: {f.dtype} {tuple(f.shape)} for a batch of {B}, C = {C}'
        table[l] = _RoiLevel(fp, h, w, ldf, float(scales[l]))
    if out is None:
        out = torch.empty((int(out_rows), P, P, C), dtype=dtype, device=boxes.device)
    else:
        assert out.dtype == dtype and tuple(out.shape) == (int(out_rows), P, P, C) and out.is_contiguous() and out.device == boxes.device
    _lib.call('hdy_roi_align_levels_fwd', ctypes.cast(table, ctypes.c_void_p), nl, C, boxes.data_ptr(), extra.data_ptr(), extra.stride(1),
              n_keep.data_ptr(), B, max_det, P, sampling_ratio, int(aligned), out.data_ptr(), int(out_rows), dcode(dtype), stream_ptr())
    return out


def mask_rows(vals, labels, mask_indices, host_indices=None):
    """vals fp32 (R, M, M, K) channels-last (possibly a channel-slice view: pitch >= K), labels int64 (R,), mask_indices int32 device table ->
    (R, 1, M, M) fp32: vals[r, :, :, mask_indices[max(labels[r], 0)]], zeros where that index is negative (hdy_mask_rows).  host_indices: the
    same table as a sequence of ints on the host, if the caller has it: an index >= K is then refused before the launch."""
    vp, R, M, M2, K, ldv = nhwc(vals)
    require_gpu(labels)
    require_gpu(mask_indices)
    assert vals.dtype == torch.float32 and M == M2, f'{vals.dtype} {tuple(vals.shape)}'
    assert labels.dtype == torch.int64 and labels.dim() == 1 and labels.numel() == R and (R <= 1 or labels.stride(0) == 1)
    assert mask_indices.dtype == torch.int32 and mask_indices.dim() == 1 and mask_indices.is_contiguous() and mask_indices.numel() >= 1
    host = None
    if host_indices is not None:
        assert len(host_indices) == mask_indices.numel()
        host = (ctypes.c_int * len(host_indices))(*[int(v) for v in host_indices])
    out = torch.empty((R, 1, M, M), dtype=torch.float32, device=vals.device)
    if R:
        _lib.call('hdy_mask_rows', vp, ldv, K, labels.data_ptr(), mask_indices.data_ptr(), ctypes.cast(host, ctypes.c_void_p) if host else None,
                  mask_indices.numel(), R, M, out.data_ptr(), out.numel(), stream_ptr())
    return out


def roi_align_bwd(dout, shape, rois, spatial_scale, sampling_ratio=2, aligned=False, into=None):
    """Scatter dout (R, P, P, C) into an fp32 image (B, H, W, C) (`into`, accumulated, or a fresh zero image)."""
    B, H, W, C = shape
    R, P = dout.shape[0], dout.shape[1]
    dfeat = torch.zeros((B, H, W, C), dtype=torch.float32, device=dout.device) if into is None else into
    rois = rois.float().contiguous()
    _lib.call('hdy_roi_align_bwd', dout.contiguous().data_ptr(), dfeat.data_ptr(), B, H, W, C, rois.data_ptr(), R, float(spatial_scale), P,
              sampling_ratio, int(aligned), dcode(dout.dtype), stream_ptr())
    return dfeat


def relu_bwd(dz, y):
    assert dz.is_contiguous() and y.is_contiguous() and dz.shape == y.shape and dz.dtype == y.dtype
    du = torch.empty_like(dz)
    _lib.call('hdy_relu_bwd', dz.data_ptr(), y.data_ptr(), du.data_ptr(), dz.numel(), dcode(dz.dtype), stream_ptr())
    return du


def cast_store(src_f32, dst, accumulate=False):
    """dst (NHWC view, any pitch) (+)= src_f32 (same logical shape, contiguous fp32)."""
    dp, N, H, W, C, ldd = nhwc(dst)
    assert src_f32.dtype == torch.float32 and src_f32.is_contiguous() and tuple(src_f32.shape) == (N, H, W, C)
    _call('hdy_cast_store', src_f32.data_ptr(), dp, ldd, N * H * W, C, int(accumulate), dcode(dst.dtype))


# ------------------------------------------------------------------------------------------ fused detection loss
class DetLossCall:
    """Pre-marshalled hdy_det_loss_ex call for one plan (pointers, geometry and the criteria's weights are static; the targets change, and
    the loss form and objectness target rule are read from det_loss on every call: gr, sort_obj_iou and a FocalLoss's gamma / alpha are
    attributes a training script may set between steps)."""

    def __init__(self, logits, gdets, na, nc, anchors_grid, balance, cls_cw, cls_pw, obj_pw, det_loss, out, device):
        nl = len(logits)
        self.nl, self.na, self.nc = nl, na, nc
        self.B = logits[0].shape[0]
        self.ny = (ctypes.c_int * nl)(*[t.shape[1] for t in logits])
        self.nx = (ctypes.c_int * nl)(*[t.shape[2] for t in logits])
        self.ldl, self.ldg = logits[0].shape[3], gdets[0].shape[3]
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.shape[3] == self.ldl for t in logits)
        assert all(g.is_contiguous() and g.shape[:3] == t.shape[:3] and g.shape[3] == self.ldg for g, t in zip(gdets, logits))
        self.lp = (ctypes.c_void_p * nl)(*[t.data_ptr() for t in logits])
        self.gp = (ctypes.c_void_p * nl)(*[g.data_ptr() for g in gdets])
        self.anc = (ctypes.c_float * (nl * na * 2))(*[float(v) for v in anchors_grid])
        self.bal = (ctypes.c_float * nl)(*[float(v) for v in list(balance)[:nl]])    # nl = 4 takes the first 4 of the 5-level table (loss.py:201)
        self.cw = (ctypes.c_float * nc)(*[float(v) for v in cls_cw])
        self.pw = (ctypes.c_float * nc)(*[float(v) for v in cls_pw])
        self.obj_pw = float(obj_pw)
        self.det_loss = det_loss
        self.hyp = det_loss.hyp
        self.dtype = dcode(gdets[0].dtype)
        self.ws, self.ws_targets, self.device = None, -1, device       # sized by the number of targets, grown when a batch has more
        self.out = out
        self.keep = (logits, gdets)

    def __call__(self, gts, tcls):
        nt = int(gts.shape[0])
        assert gts.dtype == torch.float32 and gts.is_contiguous() and (nt == 0 or gts.shape[1] == 5)
        assert tcls.dtype == torch.float32 and tcls.is_contiguous() and (nt == 0 or tuple(tcls.shape) == (nt, self.nc))
        h, dl = self.hyp, self.det_loss
        gamma, alpha = (float(dl.BCEobj.gamma), float(dl.BCEobj.alpha)) if hasattr(dl.BCEobj, 'gamma') else (0.0, 0.25)
        if nt > self.ws_targets:
            self.ws_targets = max(64, nt + nt // 2)
            nbytes = _lib.query('hdy_det_loss_workspace_bytes', self.nl, self.ny, self.nx, self.B, self.na, self.nc, self.ws_targets)
            self.ws = torch.empty(nbytes // 4 + 4, dtype=torch.float32, device=self.device)
        _lib.call('hdy_det_loss_ex', self.lp, self.ldl, self.gp, self.ldg, self.dtype, self.ny, self.nx, self.nl, self.B, self.na, self.nc,
                  self.anc, self.bal, gts.data_ptr() if nt else None, tcls.data_ptr() if nt else None, nt, self.cw, self.pw,
                  self.obj_pw, float(h['anchor_t']), float(h['label_smoothing']), float(h['box']), float(h['obj']), float(h['cls']),
                  gamma, alpha, float(dl.gr), int(bool(dl.sort_obj_iou)), self.out.data_ptr(), self.ws.data_ptr(), self.ws.numel() * 4,
                  stream_ptr())


    def mask_select(self, gts, anchors_px, strides, min_iou=0.8):
        """hdy_mask_select on this plan's logits: device tensors counts (1 + nl) int32, keep_t (nt) int64, rois (nl, nt, 5), order (nt) int64"""
        nt = int(gts.shape[0])
        dev = self.device
        counts = torch.empty(1 + self.nl, dtype=torch.int32, device=dev)
        keep_t = torch.empty(max(nt, 1), dtype=torch.int64, device=dev)
        rois = torch.empty((self.nl, max(nt, 1), 5), dtype=torch.float32, device=dev)
        order = torch.empty(max(nt, 1), dtype=torch.int64, device=dev)
        ws = torch.empty(2 * max(nt, 1), dtype=torch.int64, device=dev)
        apx = (ctypes.c_float * (self.nl * self.na * 2))(*[float(v) for v in anchors_px])
        st = (ctypes.c_float * self.nl)(*[float(v) for v in strides])
        _lib.call('hdy_mask_select', self.lp, self.ldl, self.ny, self.nx, self.nl, self.B, self.na, self.nc + 5, self.anc, apx, st,
                  gts.data_ptr() if nt else None, nt, float(self.hyp['anchor_t']), float(min_iou), counts.data_ptr(), keep_t.data_ptr(),
                  rois.data_ptr(), order.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream_ptr())
        return counts, keep_t, rois, order


def det_targets(boxes, img, labels, nc):
    """(nt, 4) clamped corner boxes, (nt,) image index, (nt,) int64 labels -> gts (nt, 5) [img, cx, cy, w, h], tcls (nt, nc) one-hot of labels 1..nc"""
    nt = int(boxes.shape[0])
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and img.dtype == torch.float32 and labels.dtype == torch.int64
    gts = torch.empty((nt, 5), dtype=torch.float32, device=boxes.device)
    tcls = torch.empty((nt, nc), dtype=torch.float32, device=boxes.device)
    _lib.call('hdy_det_targets', ptr(boxes), ptr(img), ptr(labels), nt, nc, gts.data_ptr(), tcls.data_ptr(), stream_ptr())
    return gts, tcls


def scale_inplace(t, scale):
    """t *= scale (a 1-element fp32 device tensor), no host sync"""
    assert t.is_contiguous() and scale.dtype == torch.float32 and scale.is_cuda
    _call('hdy_scale_inplace', t.data_ptr(), t.numel(), scale.data_ptr(), dcode(t.dtype))


# ------------------------------------------------------------------------------------------ segmentation branch primitives (row f4)
def groupnorm_relu_fwd(x, gamma, beta, G, eps=1e-5, relu=True):
    """x NHWC (N, H, W, C) -> (y, saved) with y = relu(GroupNorm_G(x)); saved = (stat [N][G][2], ab [N][2][C]) for the backward."""
    xp, N, H, W, C, ldx = nhwc(x)
    y = _new((N, H, W, C), x.dtype, x.device)
    stat = _new((N, G, 2), torch.float32, x.device)
    ab = _new((N, 2, C), torch.float32, x.device)
    ws = _new((_lib.query('hdy_groupnorm_workspace_floats', N, C),), torch.float32, x.device)
    _call('hdy_groupnorm_fwd', xp, ldx, ptr(gamma), ptr(beta), y.data_ptr(), C, stat.data_ptr(), ab.data_ptr(), N, H * W, C, G, float(eps),
              int(relu), dcode(x.dtype), ws.data_ptr(), ws.numel())
    return y, (stat, ab)


def groupnorm_relu_bwd(dout, x, gamma, saved, G, dgamma, dbeta, relu=True, accumulate=False):
    """Gradient of groupnorm_relu_fwd: returns dx (NHWC, x's type); dgamma / dbeta (fp32 views) are written (or accumulated)."""
    dop, N, H, W, C, lddo = nhwc(dout)
    xp, _, _, _, _, ldx = nhwc(x)
    stat, ab = saved
    dx = _new((N, H, W, C), x.dtype, x.device)
    coef = _new((N, 3, C), torch.float32, x.device)
    ws = _new((_lib.query('hdy_groupnorm_workspace_floats', N, C),), torch.float32, x.device)
    assert dout.dtype == x.dtype and dgamma.dtype == dbeta.dtype == torch.float32 and dgamma.is_contiguous() and dbeta.is_contiguous()
    _call('hdy_groupnorm_bwd', dop, lddo, xp, ldx, ptr(gamma), stat.data_ptr(), ab.data_ptr(), dx.data_ptr(), C, dgamma.data_ptr(),
              dbeta.data_ptr(), int(accumulate), coef.data_ptr(), N, H * W, C, G, int(relu), dcode(x.dtype), ws.data_ptr(), ws.numel())
    return dx


def bilinear_fwd(x, size, out=None, accumulate=False):
    """F.interpolate(x, size, mode='bilinear', align_corners=True) on NHWC; `out` (+)= when given."""
    xp, N, Hi, Wi, C, ldx = nhwc(x)
    Ho, Wo = size
    if out is None:
        out = _new((N, Ho, Wo, C), x.dtype, x.device)
        accumulate = False
    op, _, _, _, Co, ldo = nhwc(out)
    assert Co == C and tuple(out.shape[:3]) == (N, Ho, Wo) and out.dtype == x.dtype
    _call('hdy_bilinear_fwd', xp, ldx, op, ldo, N, Hi, Wi, Ho, Wo, C, int(accumulate), dcode(x.dtype))
    return out


def bilinear_bwd(dy, in_size, out=None, accumulate=False):
    dyp, N, Ho, Wo, C, lddy = nhwc(dy)
    Hi, Wi = in_size
    if out is None:
        out = _new((N, Hi, Wi, C), dy.dtype, dy.device)
        accumulate = False
    op, _, _, _, _, ldo = nhwc(out)
    if Wo >= 2 * Wi and Ho >= 2 * Hi:
        # separable: W pass over every gradient row (contiguous reads, result Wo / Wi times smaller), then the H pass
        tmp = _new((N, Ho, Wi, C), dy.dtype, dy.device)
        _call('hdy_bilinear_bwd_axis', dyp, lddy, tmp.data_ptr(), C, N * Ho, Wi, Wo, 1, C, 0, dcode(dy.dtype))
        _call('hdy_bilinear_bwd_axis', tmp.data_ptr(), C, op, ldo, N, Hi, Ho, Wi, C, int(accumulate), dcode(dy.dtype))
        return out
    _call('hdy_bilinear_bwd', dyp, lddy, op, ldo, N, Hi, Wi, Ho, Wo, C, int(accumulate), dcode(dy.dtype))
    return out


def softdice(logits, targets, class_weight=None, upstream=None, want_grad=False):
    """logits fp32 NHWC (N, H, W, ld) with nc = targets.shape[1] classes; targets fp32 (N, nc, H, W) -> (loss[1], dlogits or None)."""
    require_gpu(logits)
    N, H, W, ld = logits.shape
    nc = targets.shape[1]
    assert logits.dtype == torch.float32 and logits.is_contiguous() and targets.dtype == torch.float32 and targets.is_contiguous()
    assert tuple(targets.shape) == (N, nc, H, W) and ld >= nc
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    ws = torch.empty(_lib.query('hdy_softdice_workspace_floats', N, nc), dtype=torch.float32, device=logits.device)
    # 4-float pixels with <= 4 classes: the backward pass writes whole pixels (padding channels as zeros) — no 419 MB memset at 16 x 1280 x 1280
    dl = (torch.empty_like(logits) if ld == 4 and nc <= 4 else torch.zeros_like(logits)) if want_grad else None
    _lib.call('hdy_softdice', logits.data_ptr(), ld, targets.data_ptr(), ptr(class_weight), N, H * W, nc, loss.data_ptr(), ptr(upstream),
              ptr(dl), ld, ws.data_ptr(), ws.numel(), stream_ptr())
    return loss, dl


def softdice_wgrad_ok(logits, nc, in_w):
    """the fused loss + W-pass gradient (hdy_softdice_wgrad) covers 4-float pixels with <= 4 classes and rows that fit the LDS stage"""
    N, H, W, ld = logits.shape
    return ld == 4 and nc <= 4 and W * 16 <= 64 * 1024 and W >= 2 * in_w


def softdice_wgrad(logits, targets, class_weight, in_w, bufs=None):
    """(loss[1], dw (N, H, in_w, 4)): hdy_softdice's loss and the W pass of the resize backward of its gradient, in one launch sequence.
    bufs: a dict that keeps the three output / workspace tensors between calls (a taped backward reads `dw` at a fixed address)"""
    require_gpu(logits)
    N, H, W, ld = logits.shape
    nc = targets.shape[1]
    assert logits.dtype == torch.float32 and logits.is_contiguous() and targets.dtype == torch.float32 and targets.is_contiguous()
    assert tuple(targets.shape) == (N, nc, H, W) and softdice_wgrad_ok(logits, nc, in_w)
    key = ('softdice_wgrad', N, H, W, nc, in_w)
    if bufs is not None and bufs.get('key') == key:
        loss, ws, dw = bufs['t']
    else:
        loss = torch.empty(1, dtype=torch.float32, device=logits.device)
        ws = torch.empty(_lib.query('hdy_softdice_workspace_floats', N, nc), dtype=torch.float32, device=logits.device)
        dw = torch.empty((N, H, in_w, 4), dtype=torch.float32, device=logits.device)
        if bufs is not None:
            bufs['key'], bufs['t'] = key, (loss, ws, dw)
    _lib.call('hdy_softdice_wgrad', logits.data_ptr(), targets.data_ptr(), ptr(class_weight), N, H, W, nc, in_w, loss.data_ptr(), dw.data_ptr(),
              ws.data_ptr(), ws.numel(), stream_ptr())
    return loss, dw


def bilinear_bwd_h(dw, in_h, out, accumulate=False):
    """H pass of the resize backward: dw (N, Ho, Wi, C) -> out (N, in_h, Wi, C) (+)="""
    dp, N, Ho, Wi, C, ldd = nhwc(dw)
    op, _, _, _, _, ldo = nhwc(out)
    _call('hdy_bilinear_bwd_axis', dp, ldd, op, ldo, N, in_h, Ho, Wi, C, int(accumulate), dcode(dw.dtype))
    return out


def softmax2d(logits, nc):
    require_gpu(logits)
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    probs = torch.empty(tuple(logits.shape[:-1]) + (nc,), dtype=torch.float32, device=logits.device)
    _lib.call('hdy_softmax2d', logits.data_ptr(), logits.shape[-1], probs.data_ptr(), nc, probs.numel() // nc, nc, stream_ptr())
    return probs
