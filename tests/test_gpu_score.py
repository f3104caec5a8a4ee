"""Detection scoring on the MI355X (csrc/score.hip: hdy_ap_match, ops.ap_match, metrics.DeviceAPMeter, evaluation.score_slide,
val_nuclei.run(device_metrics=True)): the reference-made AP vectors of tests/golden/f3.npz, bit equality with the numpy restatement
(tests/score_ref.py, itself tied to APMeter by tests/test_score_host.py) on ragged batches, ties, degenerate boxes and a slide-scale set,
independence of chunk size / pruning / scratch content / input order, and the callers.  No test provokes a fault: invalid calls are answered
by status on the host (tests/test_score_host.py)."""
import ctypes
import os
import time

import numpy as np
import pytest
import torch

import score_ref as ref
from hd_yolo_amd import _lib, ops, synth
from metayolo.models.metrics import APMeter, DeviceAPMeter

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
TIME_BUDGET_S = 600            # the file's own budget: the slide-scale case is run once and the whole file must stay below this
_T0 = time.time()
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'f3.npz'), allow_pickle=False)
IOUV10 = np.linspace(0.5, 0.95, 10).astype(np.float32)
NAMES = ('hit', 'live', 'match', 'match_iou')


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_match(batch, iouv=IOUV10, ignore=(-100, -1), prow=None, trow=None, info=None):
    pb, ps, pl, poff, tb, tl, toff = batch
    out = ops.ap_match(to_dev(pb), to_dev(ps), to_dev(pl), to_dev(poff), to_dev(tb), to_dev(tl), to_dev(toff), iouv, ignore=ignore,
                       pred_row=None if prow is None else to_dev(prow.astype(np.int32)), true_row=None if trow is None else to_dev(trow.astype(np.int32)),
                       info=info)
    hit, live, match, miou = (t.cpu().numpy() for t in out)
    return hit.view(np.uint16), live, match, miou


def assert_bit_equal(got, want, what=''):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        np.testing.assert_array_equal(g, w, err_msg=f'{what} {name}')


def check(batch, iouv=IOUV10, ignore=(-100, -1), what=''):
    got = device_match(batch, iouv, ignore)
    want = ref.match_batch(*batch, iouv, ignore)
    assert_bit_equal(got, want, what)
    return got


# ------------------------------------------------------------------------------------------------ 1. the reference's own vectors
def f3_images():
    i, out = 0, []
    while f'ap_in_{i}_o_boxes' in G:
        out.append(({k: torch.from_numpy(G[f'ap_in_{i}_o_{k}']).to(DEV) for k in ('boxes', 'scores', 'labels')},
                    {k: torch.from_numpy(G[f'ap_in_{i}_t_{k}']).to(DEV) for k in ('boxes', 'labels')}))
        i += 1
    assert i == 6
    return out


@pytest.mark.parametrize('tag,ignore', [('default', (-100, -1)), ('noignore', ())])
@pytest.mark.parametrize('batched', [False, True])
def test_device_meter_reproduces_the_reference_vectors(tag, ignore, batched):
    meter = DeviceAPMeter({1: 'a', 2: 'b', 3: 'c'}, ignore=ignore)
    imgs = f3_images()
    if batched:
        meter.add_batch([o for o, _ in imgs], [t for _, t in imgs])
    else:
        for o, t in imgs:
            meter.add(o, t)
    st = meter.ap_per_class(iouv=torch.linspace(0.5, 0.95, 10), ignore=list(ignore))
    assert [int(v) for v in st['labels']] == G[f'ap_{tag}_labels'].tolist()
    assert [int(v) for v in st['counts']] == G[f'ap_{tag}_counts'].tolist()
    for k in ('ap', 'p', 'r', 'f1', 'py'):
        np.testing.assert_allclose(st[k], G[f'ap_{tag}_{k}'], rtol=1e-6, atol=1e-7, err_msg=k)


# ------------------------------------------------------------------------------------------------ 2. against the restatement
VARIANTS = {
    'default': dict(),
    'noignore': dict(ignore=()),
    'one_threshold': dict(iouv=np.array([0.5], np.float32)),
    'sixteen_thresholds': dict(iouv=np.linspace(0.5, 0.95, 16).astype(np.float32)),
    'ties': dict(gen=dict(tied_scores=True, dup_truths=True)),
    'many_ignored': dict(gen=dict(ignored=0.4)),
}


@pytest.mark.parametrize('B', [1, 7, 64])
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_random_batches_bit_equal(B, variant):
    v = VARIANTS[variant]
    rng = np.random.default_rng(1000 * B + sorted(VARIANTS).index(variant))
    batch = ref.random_batch(rng, B, 300, 400, **v.get('gen', {}))
    hit, live, match, _ = check(batch, v.get('iouv', IOUV10), v.get('ignore', (-100, -1)), f'B={B} {variant}')
    if B > 1:
        assert (match >= 0).sum() > 50 and (hit > 0).sum() > 50            # the case is not vacuous
        if variant in ('default', 'many_ignored'):
            assert (live == 0).sum() > 0


def sized_batch(rng, sizes, **kw):
    parts = [ref.random_image(rng, n, m, side=700.0, **kw) for n, m in sizes]
    cat = lambda k: np.concatenate([p[k] for p in parts])   # noqa: E731
    off = lambda c: np.concatenate(([0], np.cumsum(c))).astype(np.int32)   # noqa: E731
    return cat(0).reshape(-1, 4), cat(1), cat(2), off([s[0] for s in sizes]), cat(3).reshape(-1, 4), cat(4), off([s[1] for s in sizes])


STRADDLE = [(255, 257), (256, 256), (257, 255), (1, 1), (513, 600), (0, 300), (300, 0), (1025, 63), (64, 1030)]


def test_images_that_straddle_block_and_chunk_boundaries():
    rng = np.random.default_rng(5)
    check(sized_batch(rng, STRADDLE, tied_scores=True, dup_truths=True), what='straddle')
    check(sized_batch(rng, STRADDLE[:1]), what='one image')
    check(sized_batch(rng, [(0, 0)] * 5), what='nothing at all')


def test_degenerate_and_non_finite_boxes():
    rng = np.random.default_rng(6)
    pb, ps, pl, poff, tb, tl, toff = sized_batch(rng, [(300, 400), (600, 500), (40, 30)], dup_truths=True)
    for arr, seed in ((pb, 1), (tb, 2)):
        r = np.random.default_rng(seed)
        k = r.choice(len(arr), 60, replace=False)
        arr[k[:10], 2] = arr[k[:10], 0]                          # zero width
        arr[k[10:20], 2:] = arr[k[10:20], :2]                    # a point
        arr[k[20:30]] = arr[k[20:30]][:, [2, 3, 0, 1]]           # inverted
        arr[k[30:38], r.integers(0, 4, 8)] = np.nan
        arr[k[38:44], 2] = np.inf
        arr[k[44:50], 0] = -np.inf
        arr[k[50:54]] = np.array([-np.inf, -np.inf, np.inf, np.inf], np.float32)
        arr[k[54:60]] = 0.0                                      # zero boxes at the origin: 0 / 0
    tb[5] = pb[7] = np.array([10, 10, 10, 10], np.float32)       # identical points: inter 0, union 0
    info = {}
    got = device_match((pb, ps, pl, poff, tb, tl, toff), info=info)
    assert_bit_equal(got, ref.match_batch(pb, ps, pl, poff, tb, tl, toff, IOUV10), 'degenerate')
    assert (info['chunks_visited'], info['chunks_total']) == ref.chunk_visits(pb, poff, tb, toff, ops.AP_PRED_BLOCK, ops.AP_TRUE_CHUNK)


def test_results_do_not_depend_on_chunk_size_or_pruning():
    rng = np.random.default_rng(7)
    pb, ps, pl, poff, tb, tl, toff = sized_batch(rng, [(700, 900), (300, 1500), (1200, 200)], tied_scores=True, dup_truths=True)
    # rows in left-to-right order inside every image, so that blocks and chunks far apart exist and pruning has something to skip
    by_x = lambda b, off: np.concatenate([off[i] + np.argsort(b[off[i]:off[i + 1], 0], kind='stable') for i in range(len(off) - 1)])   # noqa: E731
    pp, tp = by_x(pb, poff), by_x(tb, toff)
    batch = (pb[pp], ps[pp], pl[pp], poff, tb[tp], tl[tp], toff)
    pb, tb = batch[0], batch[4]
    want = ref.match_batch(*batch, IOUV10)
    info = {}
    assert_bit_equal(device_match(batch, info=info), want, 'default')
    base = ref.chunk_visits(pb, poff, tb, toff, ops.AP_PRED_BLOCK, ops.AP_TRUE_CHUNK)
    assert (info['chunks_visited'], info['chunks_total']) == base and base[0] < base[1]
    for chunk in (64, 128, 256):
        with _lib.option('HDY_AP_CHUNK', chunk):
            info = {}
            assert_bit_equal(device_match(batch, info=info), want, f'chunk {chunk}')
            assert (info['chunks_visited'], info['chunks_total']) == ref.chunk_visits(pb, poff, tb, toff, ops.AP_PRED_BLOCK, chunk)
    with _lib.option('HDY_AP_NO_PRUNE', 1):
        info = {}
        assert_bit_equal(device_match(batch, info=info), want, 'no pruning')
        assert info['chunks_visited'] == info['chunks_total'] == base[1]


def test_permuted_inputs_with_rows_give_the_unpermuted_results():
    rng = np.random.default_rng(8)
    batch = ref.random_batch(rng, 9, 300, 400, tied_scores=True, dup_truths=True)
    pb, ps, pl, poff, tb, tl, toff = batch
    want = ref.match_batch(*batch, IOUV10)
    perm = lambda off: np.concatenate([off[i] + rng.permutation(off[i + 1] - off[i]) for i in range(len(off) - 1)] + [np.zeros(0, np.int64)]).astype(np.int64)   # noqa: E731
    pp, tp = perm(poff), perm(toff)                               # shuffled inside every image; row = the original position
    hit, live, match, miou = device_match((pb[pp], ps[pp], pl[pp], poff, tb[tp], tl[tp], toff), prow=pp, trow=tp)
    back = np.empty_like(pp)
    back[pp] = np.arange(len(pp))
    match = np.where(match >= 0, tp[np.maximum(match, 0)], -1).astype(np.int32)      # rows of the shuffled truth array -> original rows
    assert_bit_equal((hit[back], live[back], match[back], miou[back]), want, 'permuted')


# ------------------------------------------------------------------------------------------------ 3. the raw entry point: scratch, capacity
def raw_call(batch, ws_fill, out_fill, extra=0):
    """hdy_ap_match with caller-made outputs and workspace: `extra` rows of NaN / garbage behind off[B] on both sides, the workspace and the
    outputs filled with a byte pattern first"""
    pb, ps, pl, poff, tb, tl, toff = batch
    pad = lambda a, fill: np.concatenate([a, np.full((extra,) + a.shape[1:], fill, a.dtype)])   # noqa: E731
    d = [to_dev(x) for x in (pad(pb, np.nan), pad(ps, np.nan), pad(pl, 1), poff, pad(tb, np.nan), pad(tl, 1), toff)]
    NP, NT, B = len(ps) + extra, len(tl) + extra, len(poff) - 1
    outs = [torch.empty((NP,), dtype=dt, device=DEV) for dt in (torch.int16, torch.uint8, torch.int32, torch.float32)]
    for t in outs:
        t.view(torch.uint8).fill_(out_fill)
    wsb = _lib.query('hdy_ap_match_workspace_bytes', B, NP, NT)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=DEV)
    ws.fill_(ws_fill)
    iouv = (ctypes.c_float * 10)(*IOUV10.tolist())
    ign = (ctypes.c_longlong * 2)(-100, -1)
    _lib.call('hdy_ap_match', d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), None, NP, d[4].data_ptr(), d[5].data_ptr(),
              d[6].data_ptr(), None, NT, B, iouv, 10, 0.5, ign, 2, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
              ws.data_ptr(), wsb, ops.stream_ptr())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


def test_poisoned_workspace_and_repeats_give_identical_bits():
    rng = np.random.default_rng(9)
    batch = ref.random_batch(rng, 33, 300, 400, tied_scores=True, dup_truths=True)
    want = ref.match_batch(*batch, IOUV10)
    first = None
    for ws_fill, out_fill in ((0x00, 0x00), (0xFF, 0xFF), (0xA5, 0x5A), (0x7F, 0xFF), (0xA5, 0x5A)):
        got = raw_call(batch, ws_fill, out_fill)
        got[0] = got[0].view(np.uint16)
        assert_bit_equal(got, want, f'fill {ws_fill:#x}/{out_fill:#x}')
        if first is None:
            first = got
        for a, b in zip(got, first):
            assert a.tobytes() == b.tobytes()


def test_rows_beyond_the_last_offset_are_neither_read_nor_written():
    rng = np.random.default_rng(10)
    batch = ref.random_batch(rng, 5, 300, 400)
    n = len(batch[1])
    want = ref.match_batch(*batch, IOUV10)
    got = raw_call(batch, 0xA5, 0x5A, extra=777)
    got[0] = got[0].view(np.uint16)
    assert_bit_equal([g[:n] for g in got], want, 'padded')
    for g in got:
        assert (g[n:].view(np.uint8) == 0x5A).all()                # the fill is still there


# ------------------------------------------------------------------------------------------------ 4. the meter
def test_device_meter_surface_matches_apmeter():
    rng = np.random.default_rng(12)
    host, dev_list, dev_tuple = APMeter(), DeviceAPMeter(), DeviceAPMeter()
    for _ in range(3):                                              # three batches
        pb, ps, pl, poff, tb, tl, toff = ref.random_batch(rng, 6, 120, 150)
        outs, tgts = [], []
        for i in range(6):
            p, t = slice(poff[i], poff[i + 1]), slice(toff[i], toff[i + 1])
            outs.append({'boxes': to_dev(pb[p]), 'scores': to_dev(ps[p]), 'labels': to_dev(pl[p])})
            tgts.append({'boxes': to_dev(tb[t]), 'labels': to_dev(tl[t])})
            host.add(outs[-1], tgts[-1])
        dev_list.add_batch(outs, tgts)
        # the compacted form of device_outputs=True: rows of all images, a device n_keep, and unused capacity behind the last row
        junk = np.full((50, 4), np.nan, np.float32)
        dev_tuple.add_batch((to_dev(np.concatenate([pb, junk])), to_dev(np.concatenate([ps, junk[:, 0]])), to_dev(np.concatenate([pl, np.ones(50, np.int64)])),
                             to_dev(np.diff(poff).astype(np.int32))), tgts)
    want = host.ap_per_class(iouv=torch.linspace(0.5, 0.95, 10), ignore=[-100, -1])
    for meter in (dev_list, dev_tuple):
        assert meter.n_pred == host.n_pred and meter.n_true == host.n_true
        np.testing.assert_array_equal(meter.scores, host.scores)
        np.testing.assert_array_equal(meter.y_pred, host.y_pred)
        np.testing.assert_array_equal(meter.y_true, host.y_true)
        st = meter.ap_per_class(iouv=torch.linspace(0.5, 0.95, 10), ignore=[-100, -1])
        assert [int(v) for v in st['labels']] == [int(v) for v in want['labels']] and [int(v) for v in st['counts']] == [int(v) for v in want['counts']]
        for k in ('ap', 'p', 'r', 'f1', 'py'):
            np.testing.assert_array_equal(st[k], want[k], err_msg=k)
    with pytest.raises(ValueError):
        dev_list.ap_per_class(iouv=torch.linspace(0.5, 0.95, 5))
    with pytest.raises(ValueError):
        dev_list.ap_per_class(ignore=[])
    with pytest.raises(NotImplementedError):
        dev_list.add({'masks': 1}, {'masks': 1}, iou_type='masks')
    dev_list.reset()
    assert dev_list.n_pred == 0 and dev_list.n_true == 0 and dev_list.ap_per_class()['ap'].shape == (0, 10)


def test_stats_equal_apmeter_on_a_yolov5s_eval_batch():
    from metayolo.datasets import SyntheticTiles
    from metayolo.engines.torch_utils import to_device
    from metayolo.models.yolo import Model
    nc = 8
    model = Model(synth.make_cfg('s', nc), synth.make_hyp(conf_thres=0.02))
    model.load_state_dict(synth.synth_state_dict(synth.shapes_of(model), seed=0), strict=False)
    model = model.to(DEV).eval()
    imgs, targets = next(iter(SyntheticTiles(8, 640, nc, 1, seed=31)))
    with torch.no_grad():
        _, outputs = model(torch.stack(list(imgs)).to(DEV), compute_masks=False)
    targets = to_device(targets, DEV)
    outs, tgts = [], []
    for output, target in zip(outputs, targets):
        o, t = output['det'], dict(target['anns']['det'][0])
        t['boxes'] = t['boxes'] * 640 if t['boxes'].numel() and float(t['boxes'].max()) <= 1.0 else t['boxes']
        # the comparison is defined for distinct scores inside an image (the tie rule is the one place the two meters may differ): of equal
        # scores only the first row stays
        s = o['scores'].cpu().numpy()
        first = np.sort(np.unique(s, return_index=True)[1])
        keep = torch.from_numpy(first).to(DEV)
        outs.append({k: o[k][keep] for k in ('boxes', 'scores', 'labels')})
        tgts.append({'boxes': t['boxes'], 'labels': t['labels']})
    assert sum(len(o['scores']) for o in outs) > 100
    host, dev = APMeter(), DeviceAPMeter()
    for o, t in zip(outs, tgts):
        host.add(o, t)
    dev.add_batch(outs, tgts)
    want, st = host.ap_per_class(iouv=torch.linspace(0.5, 0.95, 10), ignore=[-100, -1]), dev.ap_per_class()
    assert [int(v) for v in st['labels']] == [int(v) for v in want['labels']] and [int(v) for v in st['counts']] == [int(v) for v in want['counts']]
    for k in ('ap', 'p', 'r', 'f1', 'py'):
        np.testing.assert_array_equal(st[k], want[k], err_msg=k)
    np.testing.assert_array_equal(dev.scores, host.scores)
    np.testing.assert_array_equal(dev.y_pred, host.y_pred)


def test_val_nuclei_device_metrics_equal_host_metrics():
    import val_nuclei
    from metayolo.datasets import SyntheticTiles
    from metayolo.models.yolo import Model
    nc = 3
    model = Model(synth.make_cfg('n', nc), synth.make_hyp(conf_thres=0.05))
    model.load_state_dict(synth.synth_state_dict(synth.shapes_of(model), seed=0), strict=False)
    model = model.to(DEV)
    res = {}
    for mode in (False, True):
        res[mode] = val_nuclei.run(model, SyntheticTiles(4, 128, nc, 3, seed=99), half=True, device_metrics=mode)
    (fit_h, stats_h, speeds_h), (fit_d, stats_d, speeds_d) = res[False], res[True]
    assert fit_h == fit_d and stats_h == stats_d and len(speeds_h) == len(speeds_d) == 3


# ------------------------------------------------------------------------------------------------ 5. slide scale, once
def test_slide_scale_set_through_score_slide():
    import evaluation
    n_objects = 190000
    tb, tl, pb, ps, pl = synth.synth_slide_truth(n_objects, 40.0 * n_objects ** 0.5, 4, seed=3)
    assert len(ps) >= 200000 and len(tl) >= 150000
    dpb, dtb = to_dev(pb), to_dev(tb)
    info = {}
    st = evaluation.score_slide({'boxes': dpb, 'scores': to_dev(ps), 'labels': to_dev(pl)}, {'boxes': dtb, 'labels': to_dev(tl)}, info=info)
    got = (st['hit'].cpu().numpy().view(np.uint16), st['live'].cpu().numpy(), st['match'].cpu().numpy(), st['match_iou'].cpu().numpy())
    want = ref.match_binned(pb, ps, pl, tb, tl, IOUV10)
    assert_bit_equal(got, want, 'slide')
    assert (want[2] >= 0).sum() > 100000 and (want[1] == 0).sum() > 1000
    # the stats are the curves of those flags
    from metayolo.models.metrics import ap_curves
    keep = want[1].astype(bool)
    flags = ((want[0][:, None] >> np.arange(10, dtype=np.uint16)[None]) & 1).astype(bool)
    curves = ap_curves(flags[keep], ps[keep], pl[keep], tl, IOUV10, [-100, -1])
    for k in ('ap', 'p', 'r', 'f1', 'py'):
        np.testing.assert_array_equal(st[k], curves[k], err_msg=k)
    # pruning: the device's count is the restated count for the order score_slide used, at the device's block and chunk size
    op, ot = (o.cpu().numpy() for o in evaluation.slide_orders(dpb, dtb))
    visited, total = ref.chunk_visits(pb[op], np.array([0, len(op)]), tb[ot], np.array([0, len(ot)]), ops.AP_PRED_BLOCK, ops.AP_TRUE_CHUNK)
    print(f'slide-scale: {len(ps)} x {len(tl)}, chunk pairs visited {info["chunks_visited"]} of {info["chunks_total"]}, restated {visited} of {total}')
    assert (info['chunks_visited'], info['chunks_total']) == (visited, total)
    assert visited < total


def test_file_time_budget():
    """last in the file: the cases above, the slide-scale one included, fit the file's own budget"""
    assert time.time() - _T0 < TIME_BUDGET_S
