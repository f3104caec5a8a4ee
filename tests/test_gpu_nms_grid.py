"""Multi-workgroup NMS of one large box set (hdy_nms_grid_begin / _round / _finish, ops.nms_grid) on the MI355X: bit-exact against the
scalar oracle and against the one-workgroup kernel, degenerate geometry, fallbacks, scale (verified by the uniqueness checker of
tests/nms_checker.py where the O(M x kept) oracle cannot follow), scratch independence, dispatch inside ops.nms and the whole-slide caller."""
import time

import numpy as np
import pytest
import torch

from hd_yolo_amd import _lib, ops, synth
from nms_checker import assert_is_greedy_nms
from oracle import nms_ref

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
TIME_BUDGET_S = 600            # the file's own budget: the scale cases are run once each and the whole file must stay below this
_T0 = time.time()
_ORACLE = {}


def dev(b, s):
    return torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).to(DEV)


def oracle(tag, b, s, thr):
    key = (tag, float(thr))
    if key not in _ORACLE:
        _ORACLE[key] = nms_ref.nms_c(b, s, thr)
    return _ORACLE[key]


def f3_set(n):
    """the construction of tests/test_gpu_f3.py::test_nms_boxes_bit_exact_order"""
    g = torch.Generator().manual_seed(n)
    c = torch.rand((n, 2), generator=g) * 300
    wh = torch.rand((n, 2), generator=g) * 40 + 4
    boxes = torch.cat([c - wh / 2, c + wh / 2], 1)
    scores = torch.rand(n, generator=g)
    scores[::7] = scores[0]                       # ties: lower index first
    return boxes.numpy(), scores.numpy()


def negative_scores_set():
    """the construction of tests/test_gpu_f3.py::test_nms_boxes_negative_scores_and_more_than_one_launch_of_survivors"""
    g = torch.Generator().manual_seed(5)
    n = 14000
    c = torch.rand((n, 2), generator=g) * 4000
    wh = torch.rand((n, 2), generator=g) * 30 + 6
    boxes = torch.cat([c - wh / 2, c + wh / 2], 1)
    scores = torch.rand(n, generator=g) * 2 - 1
    scores[::11] = scores[3]
    scores[5] = 0.0
    scores[6] = -0.0
    return boxes.numpy(), scores.numpy()


SETS = {
    'f3_1': (lambda: f3_set(1), [0.5]), 'f3_37': (lambda: f3_set(37), [0.45]), 'f3_1000': (lambda: f3_set(1000), [0.3]),
    'f3_5000': (lambda: f3_set(5000), [0.6]), 'f3_9000': (lambda: f3_set(9000), [0.45]),
    'slide_32k': (lambda: synth.synth_slide_boxes(16000, 4000, 1), [0.45, 0.2]),
    'slide_66k': (lambda: synth.synth_slide_boxes(33000, 5750, 2), [0.45, 0.2]),
    'dense_4096': (lambda: synth.synth_dense_boxes(4096, 3), [0.45, 0.2]),
    'dense_16384': (lambda: synth.synth_dense_boxes(16384, 4), [0.45, 0.2]),
    'negative_tied': (negative_scores_set, [0.4]),
}
SETS.update({f'edge_{m}': ((lambda m=m: f3_set(m)), [0.45]) for m in (2, 63, 64, 65, 8191, 8193)})
CASES = [(tag, thr) for tag, (_, thrs) in SETS.items() for thr in thrs]
_DATA = {}


def data(tag):
    if tag not in _DATA:
        _DATA[tag] = SETS[tag][0]()
    return _DATA[tag]


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize('tag,thr', CASES)
def test_bit_exact_against_the_oracle(tag, thr):
    b, s = data(tag)
    want = oracle(tag, b, s, thr)
    info = {}
    got = ops.nms_grid(*dev(b, s), thr, info=info).cpu().numpy()
    print(f'{tag} M={len(b)} thr={thr} kept={len(got)} {info}')
    assert info, 'the multi-workgroup path did not serve this set'
    assert got.dtype == np.int64 and np.array_equal(got, want)


def test_max_det_smaller_than_the_survivor_count_and_empty_set():
    b, s = data('negative_tied')
    want = oracle('negative_tied', b, s, 0.4)
    assert len(want) > 2 * 4096
    for md in (1, 300, 5000):
        got = ops.nms_grid(*dev(b, s), 0.4, max_det=md).cpu().numpy()
        assert np.array_equal(got, want[:md])
    e = ops.nms_grid(torch.zeros((0, 4), device=DEV), torch.zeros(0, device=DEV), 0.5)
    assert e.numel() == 0 and e.dtype == torch.int64


# ------------------------------------------------------------------------------------------------ 2. against the one-workgroup kernel
@pytest.mark.parametrize('tag,thr', CASES)
def test_bit_exact_against_the_one_workgroup_kernel(tag, thr):
    b, s = data(tag)
    bt, st = dev(b, s)
    info = {}
    got = ops.nms_grid(bt, st, thr, info=info)
    assert info and torch.equal(got, ops._nms_launch(bt, st, thr, len(b)))


# ------------------------------------------------------------------------------------------------ 3. degenerate geometry
def _rand_small(n, seed, side=2000.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, side, (n, 2))
    wh = rng.uniform(12, 30, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)


def _degenerate(kind):
    if kind == 'identical':
        return np.tile(np.array([[10, 20, 40, 60]], np.float32), (4096, 1)), np.random.default_rng(0).uniform(0, 1, 4096).astype(np.float32), 0.5
    if kind in ('cover_top', 'cover_bottom'):
        b, s = _rand_small(4096, 1)
        b[17] = [-50, -50, 2100, 2100]
        s[17] = 2.0 if kind == 'cover_top' else -1.0
        return b, s, 0.0 if kind == 'cover_top' else 0.3         # thr 0: the cover suppresses everything it touches
    if kind == 'improper':
        b, s = _rand_small(4096, 2, side=600.0)
        b[::5, 2] = b[::5, 0]                                     # zero width
        b[1::7, [1, 3]] = b[1::7, [3, 1]]                         # inverted
        b[2::11] = b[2::11][:, [2, 3, 0, 1]]                      # inverted both ways
        return b, s, 0.3
    if kind == 'chain':
        k = np.arange(2000, dtype=np.float32)
        b = np.stack([k * 4, np.zeros_like(k), k * 4 + 10, np.full_like(k, 10)], 1)     # IoU(k, k + 1) = 6/14, IoU(k, k + 2) = 2/18
        return b, (1.0 - k / 4000).astype(np.float32), 0.3
    if kind == 'class_offsets':
        b, s = _rand_small(4096, 3, side=640.0)
        cls = np.random.default_rng(4).integers(0, 80, 4096).astype(np.float32)
        return b + cls[:, None] * np.float32(7680), s, 0.45
    raise KeyError(kind)


@pytest.mark.parametrize('kind', ['identical', 'cover_top', 'cover_bottom', 'improper', 'chain', 'class_offsets'])
def test_degenerate_geometry(kind):
    b, s, thr = _degenerate(kind)
    want = nms_ref.nms_c(b, s, thr)
    info = {}
    got = ops.nms_grid(*dev(b, s), thr, info=info).cpu().numpy()
    print(f'{kind} M={len(b)} kept={len(got)} {info}')
    assert info and np.array_equal(got, want)
    if kind == 'identical':
        assert len(got) == 1
    if kind == 'chain':
        assert np.array_equal(got, np.arange(0, 2000, 2)) and info['rounds'] >= 1000       # the many-rounds path
    if kind == 'cover_top':
        assert got[0] == 17 and len(got) < 200
    if kind == 'class_offsets':
        assert float(b.max()) > 600000


# ------------------------------------------------------------------------------------------------ 4. fallback and argument checks
def _old_answer(bt, st, thr):
    try:
        return ops._nms_launch(bt, st, thr, bt.shape[0]), None
    except _lib.HdyError as e:
        return None, e


@pytest.mark.parametrize('what', ['nan', 'inf', 'neg_iou'])
def test_inputs_the_index_cannot_serve_are_answered_by_the_one_workgroup_kernel(what):
    b, s = _rand_small(3000, 7, side=500.0)
    thr = 0.45
    if what == 'nan':
        b[123, 1] = np.nan
    elif what == 'inf':
        b[77, 2] = np.inf
    else:
        thr = -0.1
    bt, st = dev(b, s)
    want, err = _old_answer(bt, st, thr)
    info = {}
    if err is not None:                            # the one-workgroup kernel refuses the call: so does the new entry, with the same error
        with pytest.raises(_lib.HdyError) as e:
            ops.nms_grid(bt, st, thr, info=info)
        assert str(e.value) == str(err)
    else:
        assert torch.equal(ops.nms_grid(bt, st, thr, info=info), want)
    assert not info                                # not served by the multi-workgroup path


def test_too_small_workspace_is_einval_and_writes_nothing():
    lib = _lib.load()
    M, md = 5000, 100
    need = lib.hdy_nms_grid_workspace_bytes(M)
    assert need > 0 and lib.hdy_nms_grid_workspace_bytes(M) == need and lib.hdy_nms_grid_workspace_bytes(0) == 0
    assert lib.hdy_nms_grid_workspace_bytes(M + 1) >= need
    b, s = _rand_small(M, 8)
    bs = torch.cat([t.reshape(M, -1) for t in dev(b, s)], 1).contiguous()
    ws = torch.full((need // 8 + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    keep = torch.full((md,), -77, dtype=torch.int64, device=DEV)
    stat = torch.full((4,), -77, dtype=torch.int32, device=DEV)
    small = need - 16
    assert lib.hdy_nms_grid_begin(bs.data_ptr(), M, ws.data_ptr(), small, None) == _lib.EINVAL and b'workspace' in lib.hdy_last_error()
    assert lib.hdy_nms_grid_round(M, 0.5, 0, 4, ws.data_ptr(), small, None) == _lib.EINVAL and b'workspace' in lib.hdy_last_error()
    assert lib.hdy_nms_grid_finish(M, md, keep.data_ptr(), stat.data_ptr(), stat.data_ptr() + 4, ws.data_ptr(), small, None) == _lib.EINVAL
    assert lib.hdy_nms_grid_round(M, -0.1, 0, 4, ws.data_ptr(), need, None) == _lib.EINVAL and b'iou' in lib.hdy_last_error()
    assert lib.hdy_nms_grid_begin(bs.data_ptr(), 0, ws.data_ptr(), need, None) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((ws == 0x5A5A5A5A5A5A5A5A).all()) and bool((keep == -77).all()) and bool((stat == -77).all())


# ------------------------------------------------------------------------------------------------ 5. scale
@pytest.mark.parametrize('n_objects,side', [(125000, 11000), (500000, 22000)])
def test_scale_checked_by_uniqueness_and_by_the_oracle_on_a_moated_window(n_objects, side):
    x0 = y0 = 3000.0
    x1 = y1 = 7000.0
    b, s = synth.synth_slide_boxes(n_objects, side, 11, moat=(x0, y0, x1, y1, 40.0))
    thr = 0.45
    info = {}
    t = time.time()
    got = ops.nms_grid(*dev(b, s), thr, info=info).cpu().numpy()
    print(f'M={len(b)} kept={len(got)} {info} {time.time() - t:.3f} s')
    assert info
    assert_is_greedy_nms(b, s, thr, got)
    inside = (b[:, 0] > x0) & (b[:, 1] > y0) & (b[:, 2] < x1) & (b[:, 3] < y1)
    rows = np.nonzero(inside)[0]
    assert len(rows) > 20000
    local = np.full(len(b), -1, np.int64)
    local[rows] = np.arange(len(rows))
    want = nms_ref.nms_c(b[rows], s[rows], thr)             # nothing outside the window touches a box inside it
    got_local = local[got]
    assert np.array_equal(got_local[got_local >= 0], want)


# ------------------------------------------------------------------------------------------------ 6. scratch independence and repeats
PATTERNS = {'A': 0, 'B': -1, 'C': 0x7F7F7F7F7F7F7F7F}
GUARD = 512        # int64 words behind the workspace and behind keep[max_det]


def _raw_call(bs, M, thr, md, pat):
    lib = _lib.load()
    need = lib.hdy_nms_grid_workspace_bytes(M)
    words = (need + 7) // 8
    ws = torch.full((words + GUARD,), PATTERNS[pat], dtype=torch.int64, device=DEV)
    keep = torch.full((md + GUARD,), PATTERNS[pat], dtype=torch.int64, device=DEV)
    stat = torch.full((4 + GUARD,), PATTERNS[pat] & 0x7FFFFFFF if pat == 'C' else PATTERNS[pat], dtype=torch.int32, device=DEV)
    st = ops.stream_ptr()
    _lib.call('hdy_nms_grid_begin', bs.data_ptr(), M, ws.data_ptr(), need, st)
    done = 0
    while True:
        _lib.call('hdy_nms_grid_round', M, thr, done, 16, ws.data_ptr(), need, st)
        done += 16
        _lib.call('hdy_nms_grid_finish', M, md, keep.data_ptr(), stat.data_ptr(), stat.data_ptr() + 4, ws.data_ptr(), need, st)
        n_keep, und, nonfinite, rounds = stat[:4].tolist()
        assert nonfinite == 0
        if und == 0:
            break
    assert bool((ws[words:] == PATTERNS[pat]).all()), 'bytes past ws_bytes were written'
    assert bool((keep[md:] == PATTERNS[pat]).all()), 'bytes past keep[max_det] were written'
    assert bool((stat[4:] == stat[4]).all())
    return keep[:md].clone(), n_keep, rounds


@pytest.mark.parametrize('tag,md', [('slide_32k', 40000), ('dense_16384', 1000), ('edge_8193', 8193)])
def test_scratch_independence_and_repeats(tag, md):
    b, s = data(tag)
    M = len(b)
    bs = torch.cat([t.reshape(M, -1) for t in dev(b, s)], 1).contiguous()
    want = oracle(tag, b, s, 0.45)[:md]
    first = None
    for pat in ('A', 'B', 'C', 'A', 'B', 'C'):            # three fills, six runs
        keep, n_keep, rounds = _raw_call(bs, M, 0.45, md, pat)
        assert n_keep == len(want) and np.array_equal(keep[:n_keep].cpu().numpy(), want)
        assert bool((keep[n_keep:] == -1).all())
        if first is None:
            first = (keep, n_keep)
        # (the round COUNT may differ between runs: a box that reads a neighbour's state written earlier in the same launch decides a round
        # sooner; states only move from undecided to final, so the result cannot)
        assert torch.equal(keep, first[0]) and n_keep == first[1] and rounds >= 1


# ------------------------------------------------------------------------------------------------ 7. dispatch inside ops.nms
def _spy(monkeypatch):
    calls = []
    old_launch, grid_launch = ops._nms_launch, ops._nms_grid_launch
    monkeypatch.setattr(ops, '_nms_launch', lambda *a, **k: (calls.append('one_workgroup'), old_launch(*a, **k))[1])
    monkeypatch.setattr(ops, '_nms_grid_launch', lambda *a, **k: (calls.append('grid'), grid_launch(*a, **k))[1])
    return calls


def test_dispatch_threshold(monkeypatch):
    monkeypatch.delenv('HDY_NMS_GRID_MIN', raising=False)
    assert ops.NMS_GRID_MIN >= 2000
    calls = _spy(monkeypatch)
    small = dev(*f3_set(1000))
    n_obj = ops.NMS_GRID_MIN // 2 + 2000
    b, s = synth.synth_slide_boxes(n_obj, 31.6 * n_obj ** 0.5, 5)             # the density of the slide sets above
    assert len(b) >= ops.NMS_GRID_MIN
    large = dev(b, s)
    r_small = ops.nms(*small, 0.45)
    assert calls == ['one_workgroup']
    r_large = ops.nms(*large, 0.45)
    assert calls == ['one_workgroup', 'grid']
    assert _lib.load().hdy_last_dispatch() == b'nms_grid'
    r_cut = ops.nms(*large, 0.45, max_det=777)
    assert calls[-1] == 'grid' and torch.equal(r_cut, r_large[:777])
    monkeypatch.setenv('HDY_NMS_GRID_MIN', '0')            # never
    del calls[:]
    assert torch.equal(ops.nms(*large, 0.45), r_large) and torch.equal(ops.nms(*small, 0.45), r_small)
    assert calls == ['one_workgroup', 'one_workgroup']
    monkeypatch.setenv('HDY_NMS_GRID_MIN', '256')          # read at call time
    del calls[:]
    assert torch.equal(ops.nms(*small, 0.45), r_small) and calls == ['grid']


# ------------------------------------------------------------------------------------------------ 8. the whole-slide caller
def test_inference_on_slide_is_unchanged_by_the_dispatch(monkeypatch):
    import evaluation
    from metayolo.models.yolo import Deploy, Model
    m = Model(synth.make_cfg('n', 3), synth.make_hyp(conf_thres=0.05)).to(DEV).eval()
    m.load_state_dict(synth.synth_state_dict(synth.shapes_of(m), seed=2), strict=False)
    dep = Deploy(m)
    slide = synth.synth_images(1, 448, seed=9)[0].to(DEV)
    assert len(evaluation.slide_rois(448, 448, 128, 64)) == 36
    calls = _spy(monkeypatch)
    monkeypatch.setenv('HDY_NMS_GRID_MIN', '0')
    want = evaluation.inference_on_slide(dep, slide, tile=128, overlap=64, batch_size=12)
    assert calls and 'grid' not in calls
    del calls[:]
    monkeypatch.setenv('HDY_NMS_GRID_MIN', '256')
    got = evaluation.inference_on_slide(dep, slide, tile=128, overlap=64, batch_size=12)
    assert 'grid' in calls, 'the merge did not reach the multi-workgroup path'
    assert sorted(got) == sorted(want)
    for task in want:
        assert sorted(got[task]) == sorted(want[task])
        for k, v in want[task].items():
            assert torch.equal(got[task][k], v), (task, k)
        assert len(want[task]['boxes']) > 0


def test_file_time_budget():
    """last in the file: the cases above, scale included, fit the file's own budget"""
    assert time.time() - _T0 < TIME_BUDGET_S
