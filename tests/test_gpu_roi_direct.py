"""csrc/roi.hip driven directly (ops.roi_align, ops.roi_align_bwd fresh and into=, ops.roi_align_levels, ops.cast_store, ops.relu_bwd; no
model) on an MI355X against the float64 restatement tests/roi_ref.py, on the cases of tests/roi_cases.py (tests/test_roi_ref_host.py proves
on the CPU what each contains: 1 to 3 channel blocks with a partial last one, P 1 to 28, 1 to 4 samples per bin axis, both `aligned` values,
rois over every border, outside the map, narrower than a pixel, image indices outside the batch, an image no roi names, footprints of
exactly 24x24 / 24x25 / 25x24 / 30x30, all-tiled, all-scatter and mixed sets, H == 1 and W == 1, samples exactly on the validity thresholds,
rois whose top sample leaves the closed-form footprint, batches of 1 to 1024 images for the multi-level form).

Features live in a pitched buffer at channel offset 8 (16 bytes in bf16, 32 in fp32) with 7.0 outside; the into= image, the multi-level
output and cast_store's destination are prefilled and sit between 7.0; after each call the 7.0 must be intact.

Criteria (derivations in roi_ref): every element of a forward or gradient within its first-order bound, bf16 outputs with half a bf16 ulp
on top; an image no roi names stays exactly 0 (into=: keeps its bits); two runs of an all-tiled set give equal bits wherever one roi alone
covers the pixel; the multi-level form equals the single-level calls bit for bit; cast_store and relu_bwd are exact.  relu_bwd follows
torch's CPU autograd of F.relu on every input, a NaN y included: y <= 0 ? 0 : dz lets the gradient of a NaN y through (the kernel's
earlier y > 0 ? dz : 0 returned 0 there and was changed).  No bound comes from a kernel's output and no element is excluded.

Measured on an MI355X, worst case of each group, error in units of its bound (must stay <= 1):

    group (cases)                            worst error / bound (case)                     median
    forward fp32 (23)                        0.221 (f32-4-17-1-aligned-mixed-0.0625)        0.157
    forward bf16 (23)                        0.996 (bf16-40-14-1-aligned-mixed-0.125)       0.984
    forward, NaN / inf features              0.011 (fp32) / 0.992 (bf16)
    backward, all-tiled sets (16)            0.154 (bf16-40-7-1-aligned-small-0.125)        0.095
    backward, all-scatter sets (18)          0.244 (f32-4-28-3-legacy-large-0.125)          0.131
    backward, mixed sets (12)                0.177 (bf16-40-14-1-aligned-mixed-0.125)       0.148
    backward into=, tiled (16)               0.417 (f32-72-16-2-aligned-small-0.0625)       0.174
    backward into=, scatter (18)             0.671 (bf16-72-14-4-legacy-large-0.125)        0.330
    backward into=, mixed (12)               0.593 (bf16-72-14-2-legacy-mixed-0.0625)       0.415
    backward, NaN / inf gradients (2)        0.148 (bf16-40-14-2-legacy-mixed-0.125)
    closed-form misses fp32 (7)              0.176 (x-aligned-f32)                          0.149
    closed-form misses bf16 (7)              0.984 (y-aligned-bf16)                         0.980
    multi-level fp32 (5)                     0.150 (5-7-f32)                                0.112
    multi-level bf16 (5)                     0.993 (1024-2-bf16)                            0.964
    cast_store (16), relu_bwd (4)            exact

A bf16 forward sits near 1 by construction: half a bf16 ulp is nearly all of its bound and some element always rounds that far.  The fp32
figures are what the roi arithmetic's roundings alone produce on the CPU (0.02 to 0.24 of the bound for the same cases).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import roi_cases as rc  # noqa: E402
import roi_ref as ref  # noqa: E402
from hd_yolo_amd import _lib, ops  # noqa: E402

DEV = torch.device('cuda', 0)
OFF, TAIL, PAD = 8, 8, 64
TORCH = {'f32': torch.float32, 'bf16': torch.bfloat16}
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
ALL = [(rc.case_id(c), c) for c in rc.GRID] + [(f'{n}-{dt}', (n, dt)) for dt in rc.DTYPES for n in rc.SPECIAL]
IDS, KEYS = [a for a, _ in ALL], [b for _, b in ALL]


def bits(t):
    return t.contiguous().view(INT_VIEW[t.dtype])


def figure(group, what, worst):
    print(f'ROIFIG {group} | {what} | {worst:.3f}')
    return worst


def case_of(key):
    return rc.special_case(*key) if len(key) == 2 else rc.grid_case(key)


def logged(fn):
    _lib.dispatch_log(reset=True)
    out = fn()
    torch.cuda.synchronize()
    return out, _lib.dispatch_log(reset=True)


# ------------------------------------------------------------------------------------------ buffers
class Feat:
    """[B, H, W, C] as a channel slice at OFF of a pitch C + OFF + TAIL buffer, 7.0 everywhere else"""

    def __init__(self, a, dt):
        self.C = a.shape[3]
        self.buf = torch.full(a.shape[:3] + (self.C + OFF + TAIL,), rc.POISON, dtype=TORCH[dt], device=DEV)
        self.v = self.buf[..., OFF:OFF + self.C]
        self.v.copy_(torch.from_numpy(a).to(TORCH[dt]))
        assert self.v.stride(2) == self.C + OFF + TAIL and self.v.data_ptr() % 16 == 0 and self.v.data_ptr() != self.buf.data_ptr()

    def intact(self, a):
        assert (self.buf[..., :OFF] == rc.POISON).all() and (self.buf[..., OFF + self.C:] == rc.POISON).all(), 'poison beside the features overwritten'
        assert np.array_equal(self.v.float().cpu().numpy(), a, equal_nan=True), 'the features changed'


class Flat:
    """a contiguous tensor of `shape` between PAD elements of 7.0 on either side, prefilled with `a` (or with 7.0)"""

    def __init__(self, shape, dtype, a=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), rc.POISON, dtype=dtype, device=DEV)
        self.v = self.buf[PAD:PAD + n].view(shape)
        if a is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))

    def intact(self):
        assert (self.buf[:PAD] == rc.POISON).all() and (self.buf[-PAD:] == rc.POISON).all(), 'poison around a buffer overwritten'

    def host(self):
        return self.v.float().cpu().numpy().astype(np.float64)


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(TORCH[dt]) if dt else t).to(DEV)


# ------------------------------------------------------------------------------------------ forward
def forward(c, feat=None):
    a = c['feat'] if feat is None else feat
    f = Feat(a, c['dt'])
    out, log = logged(lambda: ops.roi_align(f.v, dev(c['rois']), c['scale'], c['P'], c['S'], c['aligned']))
    assert log == ['roi_align'], log
    assert tuple(out.shape) == (len(c['rois']), c['P'], c['P'], c['C']) and out.dtype == TORCH[c['dt']]
    f.intact(a)
    want, bound = ref.roi_align_fwd(a, c['rois'], c['scale'], c['P'], c['S'], c['aligned'], with_bound=True)
    return out.float().cpu().numpy(), want, ref.finish(bound, want, c['dt'] == 'bf16')


@pytest.mark.parametrize('key', KEYS, ids=IDS)
def test_forward_matches_the_float64_restatement(key):
    c = case_of(key)
    got, want, bound = forward(c)
    figure('forward', IDS[KEYS.index(key)], ref.check(got, want, bound, 'forward'))
    dead = [r for r, b in enumerate(c['rois'][:, 0]) if not 0 <= b < c['B']]
    assert not got[dead].any()


@pytest.mark.parametrize('dt', rc.DTYPES)
def test_forward_carries_nan_and_infinity_to_exactly_the_reference_bins(dt):
    c = rc.special_case('dyadic', dt)
    got, want, bound = forward(c, rc.plant_nonfinite_features(c))
    assert np.isnan(want).any() and np.isinf(want).any()
    figure('forward nonfinite', dt, ref.check(got, want, bound, 'forward with NaN / inf features'))


# ------------------------------------------------------------------------------------------ backward
def backward(c, dout=None, into=None):
    """-> (gradient image on the host, the device tensor, dispatch log)"""
    shape = (c['B'], c['H'], c['W'], c['C'])
    d = dev(c['dout'] if dout is None else dout, c['dt'])
    rois = dev(c['rois'])
    if into is None:
        g, log = logged(lambda: ops.roi_align_bwd(d, shape, rois, c['scale'], c['S'], c['aligned']))
    else:
        buf = Flat(shape, torch.float32, into)
        g, log = logged(lambda: ops.roi_align_bwd(d, shape, rois, c['scale'], c['S'], c['aligned'], into=buf.v))
        assert g is buf.v
        buf.intact()
    assert log == ['roi_align_bwd'], log
    assert g.dtype == torch.float32 and tuple(g.shape) == shape
    return g.cpu().numpy().astype(np.float64), g, log


def classify(c):
    return rc.classify(c['rois'], c['scale'], c['P'], c['S'], c['aligned'], c['B'], c['H'], c['W'])


@pytest.mark.parametrize('key', KEYS, ids=IDS)
def test_backward_matches_the_float64_restatement(key):
    """a fresh image and into= a prefilled one; run twice"""
    c = case_of(key)
    name = IDS[KEYS.index(key)]
    shape = (c['B'], c['H'], c['W'], c['C'])
    k = classify(c)
    args = (c['dout'], shape, c['rois'], c['scale'], c['S'], c['aligned'])
    want, bound = ref.roi_align_bwd(*args, with_bound=True, tiled=k['tiled'])
    got, g1, _ = backward(c)
    kind = 'tiled' if not k['scatter'].any() else 'scatter' if not k['tiled'].any() else 'mixed'
    figure(f'backward {kind}', name, ref.check(got, want, bound, 'backward'))
    want_i, bound_i = ref.roi_align_bwd(*args, into=c['into'], with_bound=True, tiled=k['tiled'])
    got_i, gi, _ = backward(c, into=c['into'])
    figure(f'backward into {kind}', name, ref.check(got_i, want_i, bound_i, 'backward into'))
    unnamed = [b for b in range(c['B']) if b not in c['rois'][:, 0]]
    if len(key) != 2:
        assert unnamed == [rc.UNNAMED]
    for b in unnamed:                                              # exactly 0; with into=, the prefill bit for bit
        assert not g1[b].any() and torch.equal(bits(gi[b]), bits(dev(c['into'][b])))
    _, g2, _ = backward(c)
    if kind == 'tiled':                                            # one roi alone on a pixel: one atomic add onto 0, the same bits in every run
        alone = torch.from_numpy(ref.cover_count(shape, c['rois'], c['scale'], c['P'], c['S'], c['aligned']) == 1).to(DEV)
        assert bool(alone.any()) and torch.equal(bits(g1)[alone], bits(g2)[alone]), 'two runs differ where a single tiled roi writes'
    got2 = g2.cpu().numpy().astype(np.float64)
    ref.check(got2, want, bound, 'backward, second run')


@pytest.mark.parametrize('case', rc.NONFINITE_BWD, ids=rc.case_id)
def test_backward_keeps_a_nonfinite_gradient_inside_its_footprint(case):
    c = rc.grid_case(case)
    d, which = rc.plant_nonfinite_dout(c)
    shape = (c['B'], c['H'], c['W'], c['C'])
    want, bound = ref.roi_align_bwd(d, shape, c['rois'], c['scale'], c['S'], c['aligned'], with_bound=True, tiled=classify(c)['tiled'])
    may = ref.footprint_mask(shape, c['rois'], c['scale'], c['P'], c['S'], c['aligned'], which)
    got, _, _ = backward(c, dout=d)
    figure('backward nonfinite', rc.case_id(case), ref.check_bwd(got, want, bound, may, 'backward with NaN / inf gradients'))


@pytest.mark.parametrize('dt', rc.DTYPES)
@pytest.mark.parametrize('m', rc.MISSES, ids=[m[0] for m in rc.MISSES])
def test_rois_whose_top_sample_leaves_the_closed_form_footprint(m, dt):
    """the footprint comes from the samples, so these rois are ordinary ones: forward and gradient within their bounds"""
    c = rc.miss_case(m, dt)
    got, want, bound = forward(c)
    worst = ref.check(got, want, bound, 'forward')
    shape = (c['B'], c['H'], c['W'], c['C'])
    want, bound = ref.roi_align_bwd(c['dout'], shape, c['rois'], c['scale'], c['S'], c['aligned'], with_bound=True, tiled=classify(c)['tiled'])
    got, _, _ = backward(c)
    figure('closed-form misses', f'{m[0]}-{dt}', max(worst, ref.check(got, want, bound, 'backward')))


# ------------------------------------------------------------------------------------------ multi-level
def per_level(feats, c, rows):
    """Detect.attach_masks' assembly: one single-level call per level, rows put back in compacted order"""
    out = torch.zeros((len(rows), c['P'], c['P'], c['C']), dtype=feats[0].v.dtype, device=DEV)
    lv = [c['level'][r] for r in rows]
    for l, f in enumerate(feats):
        sel = [k for k, v in enumerate(lv) if -1 < v < len(feats) and int(v) == l]
        if sel:
            rois = np.array([[rows[k][0], *c['boxes'][rows[k]]] for k in sel], np.float32)
            out[sel] = ops.roi_align(f.v, dev(rois), c['scales'][l], c['P'], c['S'], False)
    return out


@pytest.mark.parametrize('dt', rc.DTYPES)
@pytest.mark.parametrize('nb,P', rc.LEVELS)
def test_levels_form_matches_the_restatement_and_the_single_level_calls(nb, P, dt):
    c = rc.levels_case(nb, P, dt)
    feats = [Feat(a, dt) for a in c['feats']]
    res = {'boxes': dev(c['boxes']), 'extra': dev(c['level'])[:, :, None].contiguous(), 'n_keep': dev(c['n_keep'])}
    all_rows, total = ref.compact_rows(c['n_keep'], rc.MAX_DET, 1 << 30)
    single = per_level(feats, c, all_rows)
    worst = 0.0
    for out_rows in sorted({max(total - 2, 1), total, total + 2}):
        want, bound, written = ref.roi_align_levels(c['feats'], c['scales'], c['boxes'], c['level'], c['n_keep'], out_rows, P, c['S'], False, 123.0)
        out = Flat((out_rows, P, P, c['C']), TORCH[dt])
        out.v.fill_(123.0)
        got, log = logged(lambda: ops.roi_align_levels([f.v for f in feats], c['scales'], res, out_rows, P, c['S'], False, out=out.v))
        assert log == ['roi_align_levels'], log
        out.intact()
        assert written == min(total, out_rows) and bool((got[written:] == 123.0).all()), 'rows behind the total were written'
        worst = max(worst, ref.check(out.host(), want, ref.finish(bound, want, dt == 'bf16'), f'levels, {out_rows} rows of {total}'))
        assert torch.equal(bits(got[:written]), bits(single[:written])), 'the multi-level form differs from the single-level calls'
    for f, a in zip(feats, c['feats']):
        f.intact(a)
    figure('levels', f'{nb}-{P}-{dt}', worst)


# ------------------------------------------------------------------------------------------ cast_store
CAST = [(35, 1), (33, 5), (7, 36), (699051, 3)]                # (pixels, channels); 699051 * 3 = 8192 * 256 + 1: the grid-stride loop


@pytest.mark.parametrize('acc', [False, True], ids=['store', 'accumulate'])
@pytest.mark.parametrize('M,C', CAST)
@pytest.mark.parametrize('dt', rc.DTYPES)
def test_cast_store_is_the_sum_rounded_once(dt, M, C, acc):
    assert M != 699051 or (M * C > 8192 * 256 and (M * C - 8192 * 256) % 2 == 1)
    g = torch.Generator().manual_seed(M + C)
    src = torch.randn((1, 1, M, C), generator=g) * 3
    old = (torch.randn((1, 1, M, C), generator=g) * 3).to(TORCH[dt])
    buf = torch.full((1, 1, M, C + 5), rc.POISON, dtype=TORCH[dt], device=DEV)
    view = buf[..., 2:2 + C]
    view.copy_(old)
    ops.cast_store(src.to(DEV), view, accumulate=acc)
    torch.cuda.synchronize()
    want = ((src + old.float()) if acc else src).to(TORCH[dt])              # the fp32 sum, rounded once
    assert torch.equal(bits(view.cpu()), bits(want))
    assert (buf[..., :2] == rc.POISON).all() and (buf[..., 2 + C:] == rc.POISON).all()


# ------------------------------------------------------------------------------------------ relu_bwd
@pytest.mark.parametrize('n', [4096, 4096 * 256 * 8 + 8 * 37], ids=['small', 'grid-stride'])
@pytest.mark.parametrize('dt', rc.DTYPES)
def test_relu_bwd_equals_torch_autograd_bit_for_bit(dt, n):
    """more than 4096 * 256 vectors in either type at the large size; y holds +0, -0, denormals, NaN and infinities, dz NaN and infinities"""
    assert n // rc.VE[dt] > 4096 * 256 or n == 4096
    g = torch.Generator().manual_seed(n % 1000)
    y = torch.randn((n,), generator=g).to(TORCH[dt])
    dz = torch.randn((n,), generator=g).to(TORCH[dt])
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, float('nan'), float('inf'), -float('inf')]).to(TORCH[dt])
    for k, at in enumerate((0, 1001, n - 14)):
        y[at:at + 7] = special
        y[at + 7:at + 14] = special
        dz[at + 7:at + 14] = torch.tensor([float('nan'), float('inf'), -float('inf'), float('nan'), float('inf'), float('nan'), float('inf')]).to(TORCH[dt])
    z = y.clone().requires_grad_(True)
    F.relu(z).backward(dz)
    got = ops.relu_bwd(dz.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(bits(got.cpu()), bits(z.grad)), 'relu_bwd differs from the CPU autograd of F.relu'
