"""csrc/detect.hip driven directly (ops.decode_level, ops.nms_batched, ops.nms, ops.det_outputs, ops.rec_det_grad_pack and, where the Python
wrappers hide an argument, the C entry points) on an MI355X against tests/detect_ref.py and oracle/nms_ref.c, on the cases of
tests/detect_cases.py (tests/test_detect_ref_host.py proves on the CPU that the restatement is the reference's decode and the eager tensor
expressions of Detect.compute_outputs, what each case contains, and that the C oracle and the numpy NMS agree on every NMS case).

Every case names in its id the kernel path it targets: decode 'tiled first branch' (no + 1 <= 16), 'tiled second branch', 'per-candidate',
'above-cap' (beyond the grid caps of either kernel); NMS 'LDS kept list' (max_det <= 4096) or 'workspace kept list'.  The decode path follows
from hdy_decode's predicate as detect_cases.takes_tiled restates it.

Criteria.  Decode: every element whose float64 reference is finite within rtol 1e-4 (the tolerance the project pins decode to) plus 1e-4 px
on the four box columns and 2^-126 on the score columns (a flushed subnormal); NaN exactly where the reference has NaN and nowhere else,
although every padding channel holds NaN; the level id exact; the rows outside [row_offset, row_offset + na ny nx) and the pads around `out`
intact in bits; the pixel-major, contiguous and permuted forms of the same values equal in bits (the kernels share one expression); no
element excluded.  NMS: keep (with its -1 padding), n_keep, boxes, scores, extra, conf and (class-aware) cls equal in bits to the oracle.
det_outputs: compacted boxes / scores / labels, the in-place scores and offsets equal in bits to the restatement, pads intact.
det_grad_pack: bits (any NaN for a NaN), padding +0, pads intact.  Errors: HDY_EINVAL, the text of hdy_last_error(), outputs untouched.

Why each of these would be noticed if reverted.  The `row > 16` branch indexing: decode cases e and f ('tiled second branch', no = 16 and 21,
11 x 13 and 6 x 10 pixels over two images) compare every element with the reference and with the per-candidate kernel's bits.  The 30000 cut:
'precut' has 31200 passing rows and 40 isolated boxes ranked from 31160 on; without the cut all 40 are kept, n_keep and keep differ from the
oracle, and the test also asserts none of them is kept.  `>=` in the size filter: in 'filter_edges' half the rows have a side exactly equal to
min_wh and pass (three values of min_wh); `>` drops them all.  Strict `>` on conf: 'strict_conf' has 1000 rows exactly at conf (three
values); `>=` keeps them.  The 256-stride prefix loop of det_outputs_kernel: the B = 300 cases need two strides for images 256..299; a
single pass misplaces every row of those images, and offsets[257..300] differ.

Findings.
  * det_outputs_kernel, NaN among the class scores.  The best-class loop started at class 0 and replaced on `v > best`, so a NaN in a LATER
    class column was skipped and a finite score elsewhere won (label = that class); torch.max, which the reference uses and the kernel's
    docstring claims to follow, returns the NaN: no hit, score = objectness, label -100.  (A NaN in the FIRST class column already agreed.)
    Before the fix all 20 single-label cases with nc = 6 failed on the rows j % 16 == 9 (score 0.95 and label 1 where the restatement has the
    objectness 1.0 and -100); the nc = 1 and multi-label cases passed.  The loop now also replaces when `v` is NaN and `best` is not: the first
    NaN wins, as torch.max.  Confirmed on the device and fixed.
  * The `row > 16` branch of decode_tile_kernel: read and run (cases e, f), nothing found.

Measured on an MI355X: error of decode in units of detect_ref.decode_bound carried to each column (decode_units; elements with a normal
fp32 reference), worst and median over the cases of each group; in brackets the same expression rounded in fp32 by numpy on the CPU
(test_detect_ref_host prints it).  A value above 1 that passes 1e-4 would be a finding about the 1-ulp assumptions.

    group (cases per fill)                  randn: worst   median      sweep: worst   median      [CPU fp32, the 12 layouts]
    tiled first branch (10)                        0.472    0.061             0.422    0.000      [randn 0.481 / 0.048]
    tiled second branch (2)                        0.481    0.060             0.297    0.000      [sweep 0.422 / 0.000]
    per-candidate (27)                             0.481    0.060             0.422    0.000
    above-cap, tiled first branch (1)              0.514    0.074
    above-cap, per-candidate (1)                   0.520    0.074

Nothing comes near 1: v_exp_f32 and v_rcp_f32 stay inside the 1-ulp model on these inputs.  The worst figures equal the CPU's because the worst
element is a box centre, whose unit is mostly the fp32 roundings of (2s - 0.5 + g) stride, the same on both; the medians show the sigmoid.
The sweep's median is 0: most of its values saturate to exactly 0 or 1.  NMS, det_outputs and det_grad_pack: bits, as stated above.

The file takes 3.2 s on an MI355X (275 tests).
"""
import ctypes
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import detect_cases as dc  # noqa: E402
import detect_ref as ref  # noqa: E402
from hd_yolo_amd import _lib, ops  # noqa: E402
from oracle import nms_ref  # noqa: E402

DEV = torch.device('cuda', 0)
TIME_BUDGET_S = 10             # 3.2 s measured on an MI355X, times three for a shared machine
_T0 = [None]                   # set when the first test of this file starts: modules are imported at collection, long before they run
PAD, PRE, POST = 64, 5, 3
SENT = -7936.0                 # sentinel of every float buffer: exact in fp32 and bf16
SENT_I = -77
_FIG, _GOT, _NMS = {}, {}, {}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def padded(n, dtype=torch.float32, fill=SENT):
    """(flat buffer with PAD elements of sentinel on both sides, the n elements between them)"""
    flat = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return flat, flat[PAD:PAD + n]


def pads_intact(flat, n, fill=SENT):
    return bool((flat[:PAD] == fill).all()) and bool((flat[PAD + n:] == fill).all())


@pytest.fixture(autouse=True, scope='module')
def _file_clock():
    _T0[0] = time.time()
    yield


# ------------------------------------------------------------------------------------------ decode
def run_decode(name, form, fill):
    """one launch of hdy_decode on the named layout; returns the level's rows (B, na ny nx, no + 1) as numpy (cached)"""
    key = (name, form, fill)
    if key in _GOT:
        return _GOT[key]
    spec, anc, st, lvl = dc.decode_setup(name)
    B, na, ny, nx, no, pitch = spec
    strides, n = dc.strides_of(form, *spec)
    shift = 1 if (name == 'misaligned' and form == 'pixel') else 0
    src = torch.full((n + 2 * PAD,), float('nan'), device=DEV)                 # padding channels and pads: NaN
    view = torch.as_strided(src, (B, na, ny, nx, no), strides + (1,), PAD + shift)
    view.copy_(torch.from_numpy(dc.decode_values(name, fill)).to(DEV))
    assert (view.data_ptr() % 16 == 0) == (shift == 0) and view.data_ptr() % 4 == 0
    rows, rpi = na * ny * nx, PRE + na * ny * nx + POST
    flat, body = padded(B * rpi * (no + 1))
    out = body.view(B, rpi, no + 1)
    ops.decode_level(view, anc, st, out, PRE, lvl)
    torch.cuda.synchronize()
    got = out[:, PRE:PRE + rows].cpu().numpy().copy()
    out[:, PRE:PRE + rows] = SENT
    assert bool((flat == SENT).all()), 'rows outside the level or the pads around out were written'
    _GOT[key] = got
    return got


def check_decode(name, fill, got, group):
    spec, anc, st, lvl = dc.decode_setup(name)
    det = dc.decode_values(name, fill)
    no = det.shape[-1]
    want = ref.decode(det, anc, st, lvl)
    g = got.astype(np.float64)
    assert np.array_equal(g[..., no], want[..., no]), 'level id'
    r, v = want[..., :no], g[..., :no]
    nan = np.isnan(r)
    assert np.isfinite(r[~nan]).all()
    assert np.array_equal(np.isnan(v), nan), 'NaN where the reference has none, or none where it has one'
    atol = np.full(no, ref.TINY)
    atol[:4] = 1e-4
    with np.errstate(invalid='ignore'):
        bad = ~nan & ~(np.abs(v - r) <= 1e-4 * np.abs(r) + atol)
    assert not bad.any(), f'{bad.sum()} elements beyond rtol 1e-4: first at {np.argwhere(bad)[0]}, got {v[bad][0]!r} for {r[bad][0]!r}'
    ratios = ref.decode_error_in_units(got, det, anc, st)
    if len(ratios):
        print(f'DETFIG {group} | {fill} | {name} | worst {ratios.max():.3f} median {np.median(ratios):.3f}')
        _FIG.setdefault((group, fill), []).append((float(ratios.max()), float(np.median(ratios))))


DECODE_CASES = [(n, f, fill) for n in dc.DECODE_LAYOUTS for f in dc.FORMS for fill in dc.FILLS]


@pytest.mark.parametrize('name,form,fill', DECODE_CASES, ids=[f'{n}-{f}-{fill}-{dc.decode_path(n, f)}'.replace(' ', '_') for n, f, fill in DECODE_CASES])
def test_decode_against_the_fp64_restatement(name, form, fill):
    check_decode(name, fill, run_decode(name, form, fill), dc.decode_path(name, form))


@pytest.mark.parametrize('name', list(dc.DECODE_LAYOUTS))
@pytest.mark.parametrize('fill', dc.FILLS)
def test_decode_tiled_and_per_candidate_rows_are_equal_in_bits(name, fill):
    assert dc.decode_path(name, 'pixel').startswith('tiled')
    tiled = run_decode(name, 'pixel', fill)
    for form in ('contig', 'permuted'):
        assert same_bits(tiled, run_decode(name, form, fill)), form


@pytest.mark.parametrize('name', list(dc.DECODE_FALLBACKS))
@pytest.mark.parametrize('fill', dc.FILLS)
def test_decode_fallbacks_per_candidate(name, fill):
    """pixel-major inputs the tiled predicate refuses (pitch above 64, pitch no multiple of 4, base not 16-byte aligned): served all the same"""
    assert dc.decode_path(name, 'pixel') == 'per-candidate'
    got = run_decode(name, 'pixel', fill)
    check_decode(name, fill, got, 'per-candidate')
    assert same_bits(got, run_decode(name, 'contig', fill))
    if name == 'misaligned':
        assert same_bits(got, run_decode('a', 'pixel', fill))                  # the tiled kernel on the aligned copy of the same values


@pytest.mark.parametrize('name,form', [('tiled', 'pixel'), ('percand', 'contig')], ids=['tiled_first_branch-above-cap', 'per-candidate-above-cap'])
def test_decode_above_cap(name, form):
    """more pixels than 2048 workgroups x 128, more candidates than 4096 x 256 threads: the grid-stride loops"""
    assert dc.decode_path(name, form) == ('tiled first branch' if name == 'tiled' else 'per-candidate')
    got = run_decode(name, form, 'randn')
    del _GOT[(name, form, 'randn')]
    check_decode(name, 'randn', got, 'above-cap ' + dc.decode_path(name, form))


# ------------------------------------------------------------------------------------------ NMS
def expected(tag, c):
    if tag not in _NMS:
        _NMS[tag] = ref.nms_expected(c['preds'], c['nc'], c['conf'], c['iou'], c['max_det'], c['min_wh'], c['class_aware'])
    return _NMS[tag]


def check_nms(tag, c):
    e = expected(tag, c)
    res = ops.nms_batched(torch.from_numpy(c['preds']).to(DEV), c['nc'], c['conf'], c['iou'], c['max_det'], min_wh=c['min_wh'],
                          class_aware=c['class_aware'])
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert np.array_equal(got['n_keep'], e['n_keep']), (got['n_keep'], e['n_keep'])
    assert np.array_equal(got['keep'], e['keep'])                               # the oracle pads with -1 too
    for b in range(c['preds'].shape[0]):
        n = int(e['n_keep'][b])
        assert (got['keep'][b, n:] == -1).all()
        for k in ('boxes', 'scores', 'extra', 'conf'):
            assert same_bits(got[k][b, :n], e[k][b]), (k, b)
        if c['class_aware']:
            assert np.array_equal(got['cls'][b, :n], e['cls'][b, :n])
    return got, e


@pytest.mark.parametrize('min_wh', dc.FILTER_MIN_WH)
def test_nms_filter_edges(min_wh):
    got, e = check_nms(('filter', min_wh), dc.nms_filter_edges(min_wh))
    assert (e['n_keep'] > 1500).all()


@pytest.mark.parametrize('conf', dc.STRICT_CONF)
def test_nms_strict_conf(conf):
    got, e = check_nms(('strict', conf), dc.nms_strict_conf(conf))
    assert 500 < e['n_keep'][0] <= 1000


@pytest.mark.parametrize('kind', dc.IOU_SETS)
@pytest.mark.parametrize('iou', [0.0, 1.0])
def test_nms_iou_threshold_ends(kind, iou):
    check_nms(('iou', kind, iou), dc.nms_iou(kind, iou))


SURV = [(M, md) for M in dc.SURVIVORS for md in dc.survivor_max_dets(M)]


@pytest.mark.parametrize('M,max_det', SURV, ids=[f'{M}-{md}-{dc.kept_list(md)}'.replace(' ', '_') for M, md in SURV])
def test_nms_survivor_counts(M, max_det):
    got, e = check_nms(('surv', M, max_det), dc.nms_survivors(M, max_det))
    if max_det == dc.NMS_LDS_KEEP + 1:                                           # LDS list and workspace list: the same common prefix
        other, _ = check_nms(('surv', M, dc.NMS_LDS_KEEP), dc.nms_survivors(M, dc.NMS_LDS_KEEP))
        n = int(min(other['n_keep'][0], got['n_keep'][0]))
        assert n >= dc.NMS_LDS_KEEP - 1 or n == got['n_keep'][0]
        assert np.array_equal(other['keep'][0, :n], got['keep'][0, :n]) and same_bits(other['boxes'][0, :n], got['boxes'][0, :n])


def test_nms_mixed_batch_of_64_and_no_rows_LDS_kept_list():
    got, e = check_nms('mixed', dc.nms_mixed_batch())
    counts = dc.mixed_counts()
    assert [int(v) for v, m in zip(got['n_keep'], counts) if m <= 0] == [0] * sum(m <= 0 for m in counts)
    got, e = check_nms('empty', dc.nms_empty_rows())
    assert (got['n_keep'] == 0).all() and (got['keep'] == -1).all()


def test_nms_class_aware_precut_LDS_kept_list():
    c, iso = dc.nms_precut()
    got, e = check_nms('precut', c)
    assert not np.isin(iso, got['keep'][0, :got['n_keep'][0]]).any()
    c2, _ = dc.nms_precut(below=True)
    got2, e2 = check_nms('precut_below', c2)
    assert np.isin(iso, got2['keep'][0, :got2['n_keep'][0]]).all()


def test_nms_class_offsets_LDS_kept_list():
    check_nms('offsets', dc.nms_class_offsets())


def test_nms_nonfinite_rows_LDS_kept_list():
    check_nms('nonfinite', dc.nms_nonfinite())


XY = [(M, md) for M in dc.SURVIVORS for md in [None] + dc.survivor_max_dets(M)[1:]]


@pytest.mark.parametrize('M,max_det', XY, ids=[f'{M}-{md}-{dc.kept_list(M if md is None else md)}'.replace(' ', '_') for M, md in XY])
def test_nms_xyxy_survivor_counts(M, max_det):
    b, s = dc.xyxy_survivors(M)
    want = nms_ref.nms_c(b, s, 0.45)
    if max_det is not None:
        want = want[:max_det]
    got = ops.nms(torch.from_numpy(b).to(DEV), torch.from_numpy(s).to(DEV), 0.45, max_det=max_det).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------ det_outputs
@pytest.mark.parametrize('B,nc,tree,edge_empty', dc.OUT_CASES)
@pytest.mark.parametrize('ml', [False, True])
@pytest.mark.parametrize('with_offsets', [False, True])
def test_det_outputs(B, nc, tree, edge_empty, ml, with_offsets):
    c = dc.det_outputs_case(B, nc, tree, edge_empty)
    want = ref.det_outputs(c['scores'], c['boxes'], c['n_keep'], c['pairs'], c['conf'], ml)
    max_det, C, T = c['max_det'], 1 + nc, B * c['max_det']
    total = int(c['n_keep'].sum())
    sflat, sbody = padded(B * max_det * C)
    scores = sbody.view(B, max_det, C)
    scores.copy_(torch.from_numpy(c['scores']).to(DEV))
    boxes = torch.from_numpy(c['boxes']).to(DEV)
    n_keep = torch.from_numpy(c['n_keep']).to(DEV)
    pairs = torch.tensor(c['pairs'], dtype=torch.int32, device=DEV).reshape(-1, 2)
    if with_offsets:
        bflat, ob = padded(T * 4)
        oflat, osc = padded(T * C if ml else T)
        lflat, ol = padded(T * C if ml else T, torch.uint8 if ml else torch.int64, 0xA5 if ml else SENT_I)
        fflat, off = padded(B + 1, torch.int32, SENT_I)
        _lib.call('hdy_det_outputs', scores.data_ptr(), boxes.data_ptr(), n_keep.data_ptr(), B, max_det, nc, pairs.data_ptr() if len(pairs) else None,
                  len(pairs), float(c['conf']), int(ml), ob.data_ptr(), osc.data_ptr(), ol.data_ptr(), off.data_ptr(), ops.stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(off.cpu().numpy(), want['offsets']) and int(off[B]) == total
        assert pads_intact(bflat, T * 4) and pads_intact(oflat, osc.numel()) and pads_intact(fflat, B + 1, SENT_I)
        assert pads_intact(lflat, ol.numel(), 0xA5 if ml else SENT_I)
        assert bool((ob[total * 4:] == SENT).all()) and bool((osc[total * (C if ml else 1):] == SENT).all())        # nothing behind the compacted rows
        assert bool((ol[total * (C if ml else 1):] == (0xA5 if ml else SENT_I)).all())
        ob, osc, ol = ob.view(T, 4), (osc.view(T, C) if ml else osc), (ol.view(T, C) if ml else ol)
    else:
        ob, osc, ol = ops.det_outputs({'scores': scores, 'boxes': boxes, 'n_keep': n_keep}, nc, c['conf'], pairs, ml)
        torch.cuda.synchronize()
    assert pads_intact(sflat, B * max_det * C)
    assert same_bits(scores.cpu().numpy(), want['scores_inplace'])                                                   # rows beyond n_keep untouched, too
    assert same_bits(ob[:total].cpu().numpy(), want['boxes'])
    gs, gl = osc[:total].cpu().numpy(), ol[:total].cpu().numpy()
    assert np.array_equal(np.isnan(gs), np.isnan(want['scores'])) and same_bits(np.where(np.isnan(gs), 0, gs), np.where(np.isnan(gs), 0, want['scores']))
    assert np.array_equal(gl.astype(np.int64), want['labels'].astype(np.int64))


# ------------------------------------------------------------------------------------------ det_grad_pack
@pytest.mark.parametrize('shape,ldo', dc.PACK_SHAPES, ids=[f'{"x".join(map(str, s))}-ld{l}' + ('-above-cap' if l == 43 else '') for s, l in dc.PACK_SHAPES])
@pytest.mark.parametrize('form', dc.PACK_FORMS)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_det_grad_pack(shape, ldo, form, dt):
    B, na, ny, nx, no = shape
    vals = torch.from_numpy(dc.grad_pack_values(shape)).to(DEV)
    if form == 'pixel':
        g = vals.permute(0, 2, 3, 1, 4).contiguous().permute(0, 3, 1, 2, 4)
    elif form == 'contig':
        g = vals.contiguous()
    else:
        g = torch.full(shape + (2,), float('nan'), device=DEV)
        g[..., 0] = vals
        g = g[..., 0]
        assert g.stride(4) == 2
    dtype = torch.float32 if dt == 'f32' else torch.bfloat16
    n = B * ny * nx * ldo
    flat, body = padded(n, dtype)
    out = body.view(B, ny, nx, ldo)
    ops.run([ops.rec_det_grad_pack(g, out, na, no)])
    torch.cuda.synchronize()
    assert pads_intact(flat, n)
    got = out.float().cpu().numpy()
    want = ref.grad_pack(dc.grad_pack_values(shape), na, no, ldo, dt)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert same_bits(np.where(nan, 0, got), np.where(nan, 0, want))
    assert (u32(got[..., na * no:]) == 0).all()                                   # +0


# ------------------------------------------------------------------------------------------ argument errors
def _einval(rc, *words):
    text = _lib.load().hdy_last_error()
    assert rc == _lib.EINVAL, (rc, text)
    assert all(w in text for w in words), text


def test_decode_argument_errors_write_nothing():
    lib = _lib.load()
    B, na, ny, nx, no = 2, 3, 4, 5, 7
    det = torch.zeros((B, na, ny, nx, no), device=DEV)
    anc = (ctypes.c_float * 16)(*([4.0] * 16))
    ap = ctypes.cast(anc, ctypes.c_void_p)
    rpi = na * ny * nx
    flat, body = padded(B * rpi * (no + 1))
    s = det.stride()

    def call(**kw):
        a = dict(det=det.data_ptr(), out=body.data_ptr(), row_offset=0, rpi=rpi, B=B, na=na, ny=ny, nx=nx, no=no)
        a.update(kw)
        return lib.hdy_decode(a['det'], s[0], s[1], s[2], s[3], ap, 8.0, a['out'], a['row_offset'], a['rpi'], 0, a['B'], a['na'], a['ny'], a['nx'],
                              a['no'], ops.stream_ptr())
    _einval(call(na=9), b'bad shape', b'na=9')
    _einval(call(na=0), b'bad shape')
    _einval(call(no=4), b'bad shape', b'no=4')
    _einval(call(B=0), b'bad shape')
    _einval(call(ny=0), b'bad shape')
    _einval(call(row_offset=1), b'does not fit')
    _einval(call(row_offset=-1), b'does not fit')
    _einval(call(rpi=rpi - 1), b'does not fit')
    _einval(call(det=None), b'null')
    _einval(call(out=None), b'null')
    torch.cuda.synchronize()
    assert bool((flat == SENT).all())


def test_nms_argument_errors_write_nothing():
    lib = _lib.load()
    B, N, nc = 2, 100, 2
    row = 5 + nc + 1
    preds = torch.from_numpy(dc._rows(np.random.default_rng(0), B * N, nc, 300.0).reshape(B, N, row)).to(DEV)
    outs = {}

    def bufs(md):
        if md not in outs:
            wsb = lib.hdy_nms_workspace_bytes_for(B, N, md)
            outs[md] = dict(keep=torch.full((B, md), SENT_I, dtype=torch.int64, device=DEV), n_keep=torch.full((B,), SENT_I, dtype=torch.int32, device=DEV),
                            boxes=torch.full((B, md, 4), SENT, device=DEV), scores=torch.full((B, md, 1 + nc), SENT, device=DEV),
                            extra=torch.full((B, md, 1), SENT, device=DEV), conf=torch.full((B, md), SENT, device=DEV),
                            cls=torch.full((B, md), SENT_I, dtype=torch.int32, device=DEV),
                            ws=torch.full(((wsb + 15) // 16 * 2,), SENT_I, dtype=torch.int64, device=DEV), wsb=wsb)
        return outs[md]

    def call(md=300, **kw):
        o = bufs(md)
        a = dict(B=B, N=N, row=row, nc=nc, conf=0.25, iou=0.45, max_det=md, extra=o['extra'].data_ptr(), ws_bytes=o['ws'].numel() * 8, keep=o['keep'].data_ptr())
        a.update(kw)
        return lib.hdy_nms_batched(preds.data_ptr(), a['B'], a['N'], a['row'], a['nc'], a['conf'], a['iou'], a['max_det'], 2.0, 0, a['keep'],
                                   o['n_keep'].data_ptr(), o['boxes'].data_ptr(), o['scores'].data_ptr(), a['extra'], o['conf'].data_ptr(),
                                   o['cls'].data_ptr(), o['ws'].data_ptr(), a['ws_bytes'], ops.stream_ptr())
    for v in (-0.1, 1.5, float('nan')):
        _einval(call(conf=v), b'thresholds')
        _einval(call(iou=v), b'thresholds')
    _einval(call(row=5 + nc - 1), b'too short')
    _einval(call(nc=0), b'too short')
    _einval(call(extra=None), b'out_extra')
    _einval(call(max_det=0), b'max_det')
    _einval(call(B=-1), b'negative')
    _einval(call(N=-1), b'negative')
    _einval(call(keep=None), b'null output')
    for md in (dc.NMS_LDS_KEEP, dc.NMS_LDS_KEEP + 1):
        need = bufs(md)['wsb']
        assert need == lib.hdy_nms_workspace_bytes_for(B, N, md) and (md <= dc.NMS_LDS_KEEP or need >= B * md * 20)
        _einval(call(md, ws_bytes=need - 1), b'workspace too small')
        # hdy_nms_boxes: the same workspace rule
        assert lib.hdy_nms_boxes(preds.data_ptr(), B, N, 0.45, md, bufs(md)['keep'].data_ptr(), bufs(md)['n_keep'].data_ptr(), bufs(md)['ws'].data_ptr(),
                                 need - 1, ops.stream_ptr()) == _lib.EINVAL and b'workspace too small' in lib.hdy_last_error()
    o = bufs(300)
    for bad_iou in (-0.1, 1.5):
        assert lib.hdy_nms_boxes(preds.data_ptr(), B, N, bad_iou, 300, o['keep'].data_ptr(), o['n_keep'].data_ptr(), o['ws'].data_ptr(), o['ws'].numel() * 8,
                                 ops.stream_ptr()) == _lib.EINVAL and b'iou' in lib.hdy_last_error()
    assert lib.hdy_nms_boxes(preds.data_ptr(), B, N, 0.45, 0, o['keep'].data_ptr(), o['n_keep'].data_ptr(), o['ws'].data_ptr(), o['ws'].numel() * 8,
                             ops.stream_ptr()) == _lib.EINVAL and b'max_det' in lib.hdy_last_error()
    assert lib.hdy_nms_boxes(preds.data_ptr(), B, N, 0.45, 300, None, o['n_keep'].data_ptr(), o['ws'].data_ptr(), o['ws'].numel() * 8,
                             ops.stream_ptr()) == _lib.EINVAL and b'null' in lib.hdy_last_error()
    torch.cuda.synchronize()
    for o in outs.values():
        for k in ('keep', 'n_keep', 'cls', 'ws'):
            assert bool((o[k] == SENT_I).all()), k
        for k in ('boxes', 'scores', 'extra', 'conf'):
            assert bool((o[k] == SENT).all()), k


def test_det_outputs_and_grad_pack_argument_errors_write_nothing():
    lib = _lib.load()
    B, md, nc = 3, 4, 2
    scores = torch.full((B, md, 1 + nc), 0.5, device=DEV)
    boxes = torch.zeros((B, md, 4), device=DEV)
    n_keep = torch.full((B,), md, dtype=torch.int32, device=DEV)
    ob, osc = torch.full((B * md, 4), SENT, device=DEV), torch.full((B * md,), SENT, device=DEV)
    ol = torch.full((B * md,), SENT_I, dtype=torch.int64, device=DEV)
    pairs = torch.tensor([[1, 0]], dtype=torch.int32, device=DEV)

    def call(**kw):
        a = dict(B=B, md=md, nc=nc, pairs=pairs.data_ptr(), npairs=1, scores=scores.data_ptr(), labels=ol.data_ptr())
        a.update(kw)
        return lib.hdy_det_outputs(a['scores'], boxes.data_ptr(), n_keep.data_ptr(), a['B'], a['md'], a['nc'], a['pairs'], a['npairs'], 0.2, 0,
                                   ob.data_ptr(), osc.data_ptr(), a['labels'], None, ops.stream_ptr())
    _einval(call(B=-1), b'bad sizes')
    _einval(call(md=0), b'bad sizes')
    _einval(call(nc=0), b'bad sizes')
    _einval(call(npairs=-1), b'bad sizes')
    _einval(call(pairs=None), b'null')
    _einval(call(scores=None), b'null')
    _einval(call(labels=None), b'null')
    g = torch.ones((1, 3, 2, 2, 5), device=DEV)
    out = torch.full((1, 2, 2, 16), SENT, device=DEV)
    s = g.stride()
    for ldo, na in ((14, 3), (16, 0)):
        _einval(lib.hdy_det_grad_pack(g.data_ptr(), s[0], s[1], s[2], s[3], s[4], out.data_ptr(), ldo, 1, na, 2, 2, 5, _lib.F32, ops.stream_ptr()), b'bad args')
    _einval(lib.hdy_det_grad_pack(g.data_ptr(), s[0], s[1], s[2], s[3], s[4], None, 16, 1, 3, 2, 2, 5, _lib.F32, ops.stream_ptr()), b'bad args')
    torch.cuda.synchronize()
    assert bool((scores == 0.5).all()) and bool((ob == SENT).all()) and bool((osc == SENT).all()) and bool((ol == SENT_I).all()) and bool((out == SENT).all())


# ------------------------------------------------------------------------------------------ figures and time
def test_report_decode_figures():
    """the table of the module docstring, from the cases above"""
    for (group, fill), v in sorted(_FIG.items()):
        worst, med = max(w for w, _ in v), float(np.median([m for _, m in v]))
        print(f'DETFIG TABLE {group} | {fill} | {len(v)} cases | worst {worst:.3f} | median {med:.3f}')


def test_file_time_budget():
    """last in the file: the cases above fit the file's own budget"""
    print(f'DETFIG file time {time.time() - _T0[0]:.1f} s')
    assert time.time() - _T0[0] < TIME_BUDGET_S
