"""Host side of the mask scoring (csrc/mask_score.hip), no GPU: metrics.get_mask_ious and the host APMeter's iou_type='masks' against the
reference's own results (tests/golden/mask_ap.npz, made by tests/golden/make_golden_mask_ap.py), the numpy restatement (tests/mask_score_ref.py)
against both, the stated tie rules, the construction that turns a label map back into paste inputs, and the ABI surface of the two entry
points (invalid calls answered by status and message before anything is dereferenced or launched)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mask_score_ref as ref
import paste_ref
from hd_yolo_amd import _lib, build
from metayolo.models import metrics

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
IOUV = torch.linspace(0.5, 0.95, 10)


@pytest.fixture(scope='module')
def golden():
    g = np.load(os.path.join(HERE, 'golden', 'mask_ap.npz'))
    images = []
    for i in range(int(g['n_images'])):
        images.append(dict(pred_map=g[f'pred_map_{i}'].astype(np.int32), true_map=g[f'true_map_{i}'].astype(np.int32), scores=g[f'scores_{i}'],
                           pred_labels=g[f'pred_labels_{i}'], true_labels=g[f'true_labels_{i}'], ious=g[f'ious_{i}']))
    return g, images


def host_meter(images):
    meter = metrics.APMeter()
    for im in images:
        n, m = len(im['scores']), len(im['true_labels'])
        meter.add({'scores': torch.from_numpy(im['scores']), 'labels': torch.from_numpy(im['pred_labels']),
                   'masks': torch.from_numpy(ref.dense_masks(im['pred_map'], n))},
                  {'labels': torch.from_numpy(im['true_labels']), 'masks': torch.from_numpy(ref.dense_masks(im['true_map'], m))}, iou_type='masks')
    return meter


def test_the_golden_holds_what_the_issue_asks(golden):
    g, images = golden
    assert len(images) == 3 and len(g['seeds_tried']) >= 1
    sourced = passing = 0
    for im in images:
        assert im['pred_map'].shape == im['true_map'].shape == (64, 64) and 10 <= len(im['true_labels']) <= 25
        assert len(np.unique(im['scores'])) == len(im['scores'])
        passing += int((im['ious'] >= 0.5).sum())
        sourced += len(im['scores'])
    every = np.concatenate([im['scores'] for im in images])
    assert len(np.unique(every)) == len(every)
    assert passing * 2 > sourced                                     # most predictions have a pair
    assert any((im['true_labels'] == -1).any() for im in images)      # an ignored label is in use
    # inputs and IoUs are a few KB; the rest of the file is the reference's four (3, 1000) float64 curves, compared bit for bit below
    assert sum(g[k].nbytes for k in g.files if k not in ('py', 'p', 'r', 'f1')) < 32 * 1024
    assert os.path.getsize(os.path.join(HERE, 'golden', 'mask_ap.npz')) < 100 * 1024


def test_get_mask_ious_equals_the_reference_bit_for_bit(golden):
    _, images = golden
    for im in images:
        n, m = len(im['scores']), len(im['true_labels'])
        got = metrics.get_mask_ious(torch.from_numpy(ref.dense_masks(im['pred_map'], n)), torch.from_numpy(ref.dense_masks(im['true_map'], m)))
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, m)
        assert got.numpy().tobytes() == im['ious'].tobytes()
        # (n, 1, H, W) masks, as the mask paste delivers them, are the same masks
        again = metrics.get_mask_ious(torch.from_numpy(ref.dense_masks(im['pred_map'], n))[:, None], torch.from_numpy(ref.dense_masks(im['true_map'], m)))
        assert torch.equal(got, again)


def test_the_stated_iou_from_integer_counts_equals_the_reference_bit_for_bit(golden):
    """float32(inter) / float32(area_p + area_t - inter): the reference's '+ 1e-8' vanishes in fp32 once the union is >= 1"""
    _, images = golden
    for im in images:
        pairs, pa, ta = ref.overlap(im['pred_map'], im['true_map'], len(im['scores']), len(im['true_labels']))
        assert (pa > 0).all() and (ta > 0).all()
        assert ref.iou_matrix(pairs, pa, ta).tobytes() == im['ious'].tobytes()


def test_host_apmeter_masks_equals_the_reference_bit_for_bit(golden):
    g, images = golden
    st = host_meter(images).ap_per_class(iouv=IOUV)
    assert np.array_equal(np.array(st['labels']), g['labels']) and np.array_equal(np.array(st['counts']), g['counts'])
    for k in ('ap', 'p', 'r', 'f1', 'py'):
        np.testing.assert_array_equal(np.asarray(st[k], np.float64), g[k], err_msg=k)


def test_restatement_equals_host_apmeter_on_the_golden_inputs(golden):
    _, images = golden
    rm = ref.RefMeter(iouv=IOUV.numpy())
    for im in images:
        rm.add(im['pred_map'], im['scores'], im['pred_labels'], im['true_map'], im['true_labels'])
    want, got = host_meter(images).ap_per_class(iouv=IOUV), rm.ap_per_class()
    assert list(got['labels']) == list(want['labels']) and list(got['counts']) == list(want['counts'])
    for k in ('ap', 'p', 'r', 'f1', 'py'):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_restatement_overlap_known_answers():
    pm = np.array([[0, 0, -1, 1], [0, 2, 2, 1], [-1, 2, 7, 65535]], np.int32)
    tm = np.array([[0, 1, 1, 1], [0, 1, -7, 3], [0, 1, 1, 1]], np.int32)
    pairs, pa, ta = ref.overlap(pm, tm, 3, 2)                         # 7, 65535 and label 3 are background
    assert pairs.tolist() == [[0, 0, 2], [0, 1, 1], [1, 1, 1], [2, 1, 2]]
    assert pa.tolist() == [3, 2, 3] and ta.tolist() == [3, 7]
    assert ref.pair_ious(pairs, pa, ta).tolist() == [f32(2) / f32(4), f32(1) / f32(9), f32(1) / f32(8), f32(2) / f32(8)]
    # segments: two 1 x 4 tiles whose local rows are shifted by the bases
    pairs, pa, ta = ref.overlap(np.array([[0, 0, 1, -1], [0, 1, 1, -1]]), np.array([[0, 0, 0, 0], [0, 0, -1, 1]]), 4, 3, [0, 2], [0, 1])
    assert pairs.tolist() == [[0, 0, 2], [1, 0, 1], [2, 1, 1], [3, 1, 1]] and pa.tolist() == [2, 1, 1, 2] and ta.tolist() == [4, 2, 1]


def test_tie_rules_of_the_restatement():
    """rule 2: two truths with the same IoU for one prediction -> the lowest truth row; rule 3: two predictions with equal scores on one
    truth -> the lower prediction row; both follow pred_row / true_row when given."""
    iouv = IOUV.numpy()
    # prediction 0 covers 4 + 4 pixels of truths 0 and 1 (4 pixels each) and nothing else: IoU 4 / 8 with both
    pairs, pa, ta = np.array([[0, 0, 4], [0, 1, 4]]), np.array([8], np.int32), np.array([4, 4], np.int32)
    hit, live, match, miou = ref.match(pairs, pa, ta, [0.9], [1], [1, 1], iouv)
    assert match.tolist() == [0] and miou.tolist() == [0.5] and hit.tolist() == [1] and live.tolist() == [1]
    assert ref.match(pairs, pa, ta, [0.9], [1], [1, 1], iouv, trow=[5, 2])[2].tolist() == [1]
    # predictions 0 and 1 share truth 0 with equal scores; prediction 1 has the higher IoU, which plays no part in rule 3
    pairs, pa, ta = np.array([[0, 0, 3], [1, 0, 6]]), np.array([3, 6], np.int32), np.array([9], np.int32)
    hit, live, match, miou = ref.match(pairs, pa, ta, [0.5, 0.5], [1, 1], [1], iouv, pair_iou=0.3)
    assert match.tolist() == [0, -1] and miou.tolist() == [f32(3) / f32(9), 0]
    assert ref.match(pairs, pa, ta, [0.5, 0.5], [1, 1], [1], iouv, pair_iou=0.3, prow=[3, 1])[2].tolist() == [-1, 0]
    # an ignored truth only touches: the prediction leaves the curves; an ignored prediction alike; a label disagreement stays live, unmatched
    pairs, pa, ta = np.array([[0, 0, 4], [1, 1, 4], [2, 2, 4]]), np.array([4, 4, 4], np.int32), np.array([4, 4, 4], np.int32)
    hit, live, match, _ = ref.match(pairs, pa, ta, [0.9, 0.8, 0.7], [1, -1, 2], [-1, 1, 1], iouv)
    assert live.tolist() == [0, 0, 1] and match.tolist() == [-1, -1, -1] and hit.tolist() == [0, 0, 0]


def test_paste_inputs_give_the_label_map_back():
    """the construction the device tests and the evaluation CLI rely on: boxes that expand to exactly P x P integer boxes make the paste's
    resize the identity; checked through the paste restatement (tests/paste_ref.py), canvas borders and negative origins included"""
    rng = np.random.default_rng(3)
    for shape in ((64, 64), (37, 61)):
        pm, tm, n_pred, _ = ref.ellipse_pair(rng, shape, 14)
        for lm, n in ((pm, n_pred), (tm, 14)):
            masks, boxes = ref.paste_inputs(lm, n)
            got = paste_ref.label_map(masks[:, 0], boxes, (0, 0, shape[1], shape[0]), 0.5, padding=1)
            assert np.array_equal(got, lm)


# ---- the ABI surface, through the built library -------------------------------------------------------------------------------------------
FAKE = 0x10000      # an aligned non-NULL "device pointer": every call below must fail validation before anything dereferences or launches


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_abi_revision_and_registration(lib):
    assert lib.hdy_version() == _lib.ABI_VERSION >= 13
    for name in ('hdy_label_overlap', 'hdy_mask_ap_match'):
        assert name in _lib.SIGNATURES and lib.hdy_exec_op(name.encode()) >= 0
    assert lib.hdy_label_overlap_workspace_bytes(64) == 64 * 12 and lib.hdy_label_overlap_workspace_bytes(1 << 20) == (1 << 20) * 12
    for bad in (0, -8, 48, 100, 1 << 31):
        assert lib.hdy_label_overlap_workspace_bytes(bad) == 0
    assert lib.hdy_mask_ap_match_workspace_bytes(100, 50) >= 150 * 8 and lib.hdy_mask_ap_match_workspace_bytes(0, 0) > 0
    assert lib.hdy_mask_ap_match_workspace_bytes(-1, 0) == 0


def test_label_overlap_argument_checks(lib):
    def call(pm=FAKE, tm=FAKE, elems=4096, seg_elems=0, n_seg=0, pbase=None, tbase=None, n_pred=40, n_true=35, parea=FAKE, tarea=FAKE, table=FAKE,
             table_bytes=None, slots=256, status=FAKE):
        tb = lib.hdy_label_overlap_workspace_bytes(slots) if table_bytes is None else table_bytes
        return lib.hdy_label_overlap(pm, tm, elems, seg_elems, n_seg, pbase, tbase, n_pred, n_true, parea, tarea, table, tb, slots, status, None), \
            lib.hdy_last_error()

    for kw in ({'pm': None}, {'tm': None}, {'parea': None}, {'tarea': None}, {'table': None}, {'status': None}):
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and b'null' in msg, kw
    for s in (0, 100, 48, -64, 1 << 31):
        rc, msg = call(slots=s, table_bytes=1 << 40)
        assert rc == _lib.EINVAL and b'power of two' in msg, s
    rc, msg = call(table_bytes=256 * 12 - 1)
    assert rc == _lib.EINVAL and b'too small' in msg
    assert call(elems=-1)[0] == _lib.EINVAL and call(n_pred=-1)[0] == _lib.EINVAL and call(n_true=-3)[0] == _lib.EINVAL
    rc, msg = call(n_seg=4, seg_elems=1024)
    assert rc == _lib.EINVAL and b'null segment base' in msg
    for seg_elems in (1000, 0, -1024):
        rc, msg = call(n_seg=4, seg_elems=seg_elems, pbase=FAKE, tbase=FAKE)
        assert rc == _lib.EINVAL and b'n_seg * seg_elems' in msg
    # 64-bit sizes: the product that 32-bit arithmetic would accept is refused
    rc, msg = call(n_seg=70000, seg_elems=70000, pbase=FAKE, tbase=FAKE, elems=(70000 * 70000) & 0xFFFFFFFF)
    assert rc == _lib.EINVAL and b'n_seg * seg_elems' in msg
    assert call(pm=FAKE + 2)[0] == _lib.EINVAL and call(table=FAKE + 8)[0] == _lib.EINVAL


RULES = dict(ps=FAKE, pl=FAKE, tl=FAKE, n_iou=10, pair_iou=0.5, n_ign=2, hit=FAKE, live=FAKE, match=FAKE, miou=FAKE)


def _rule_arrays(a):
    a.setdefault('iouv', (ctypes.c_float * 17)(*np.linspace(0.5, 0.95, 17).tolist()))
    a.setdefault('ignore', (ctypes.c_longlong * 5)(-100, -1, 7, 8, 9))
    return a


def _box_rules(lib, **kw):
    a = _rule_arrays(dict(RULES, **kw))
    rc = lib.hdy_ap_match(FAKE, a['ps'], a['pl'], FAKE, None, 40, FAKE, a['tl'], FAKE, None, 35, 2, a['iouv'], a['n_iou'], a['pair_iou'], a['ignore'],
                          a['n_ign'], a['hit'], a['live'], a['match'], a['miou'], FAKE, lib.hdy_ap_match_workspace_bytes(2, 40, 35), None)
    return rc, lib.hdy_last_error()


def _mask_rules(lib, **kw):
    a = _rule_arrays(dict(RULES, **kw))
    rc = lib.hdy_mask_ap_match(FAKE, lib.hdy_label_overlap_workspace_bytes(256), 256, FAKE, FAKE, a['ps'], a['pl'], None, 40, a['tl'], None, 35, a['iouv'],
                               a['n_iou'], a['pair_iou'], a['ignore'], a['n_ign'], a['hit'], a['live'], a['match'], a['miou'], FAKE,
                               lib.hdy_mask_ap_match_workspace_bytes(40, 35), None)
    return rc, lib.hdy_last_error()


@pytest.mark.parametrize('call', [_box_rules, _mask_rules], ids=['ap_match', 'mask_ap_match'])
def test_the_rule_checks_both_matchers_share(lib, call):
    """the checks of csrc/ap_common.h (ap_check_rules), through hdy_ap_match and hdy_mask_ap_match: the same invalid rule block is refused by
    both with the same words, before any launch"""
    lib.hdy_dispatch_log_reset()
    for name in ('iouv', 'ignore', 'hit', 'live', 'match', 'miou', 'ps', 'pl'):
        rc, msg = call(lib, **{name: None})
        assert rc == _lib.EINVAL and b'null' in msg, name
    for n in (0, 17, -1):
        rc, msg = call(lib, n_iou=n)
        assert rc == _lib.EINVAL and b'n_iou=' in msg and b'[1, 16]' in msg, n
    rc, msg = call(lib, n_ign=5)
    assert rc == _lib.EINVAL and b'n_ignore=5' in msg
    for v in (0.0, 1.5, float('nan')):
        rc, msg = call(lib, pair_iou=v)
        assert rc == _lib.EINVAL and b'pair_iou' in msg, v
    for kw in ({'pl': FAKE + 4}, {'hit': FAKE + 1}):
        rc, msg = call(lib, **kw)
        assert rc == _lib.EINVAL and b'aligned' in msg, kw
    assert _lib.dispatch_log() == []


def test_mask_ap_match_argument_checks(lib):
    thr = (ctypes.c_float * 17)(*np.linspace(0.5, 0.95, 17).tolist())
    ign = (ctypes.c_longlong * 5)(-100, -1, 7, 8, 9)

    def call(table=FAKE, table_bytes=None, slots=256, parea=FAKE, tarea=FAKE, ps=FAKE, pl=FAKE, prow=None, n_pred=40, tl=FAKE, trow=None, n_true=35,
             iouv=thr, n_iou=10, pair_iou=0.5, ignore=ign, n_ign=2, hit=FAKE, live=FAKE, match=FAKE, miou=FAKE, ws=FAKE, ws_bytes=None):
        tb = lib.hdy_label_overlap_workspace_bytes(slots) if table_bytes is None else table_bytes
        wb = lib.hdy_mask_ap_match_workspace_bytes(n_pred, n_true) if ws_bytes is None else ws_bytes
        return lib.hdy_mask_ap_match(table, tb, slots, parea, tarea, ps, pl, prow, n_pred, tl, trow, n_true, iouv, n_iou, pair_iou, ignore, n_ign, hit,
                                     live, match, miou, ws, wb, None), lib.hdy_last_error()

    for kw in ({'table': None}, {'parea': None}, {'tarea': None}, {'ps': None}, {'pl': None}, {'tl': None}, {'iouv': None}, {'ignore': None},
               {'hit': None}, {'live': None}, {'match': None}, {'miou': None}, {'ws': None}):
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and b'null' in msg, kw
    for n in (0, 17, -1):
        rc, msg = call(n_iou=n)
        assert rc == _lib.EINVAL and b'n_iou=' in msg and b'[1, 16]' in msg
    rc, msg = call(n_ign=5)
    assert rc == _lib.EINVAL and b'n_ignore=5' in msg
    for s in (0, 100, -256):
        rc, msg = call(slots=s, table_bytes=1 << 40)
        assert rc == _lib.EINVAL and b'power of two' in msg
    rc, msg = call(table_bytes=256 * 12 - 4)
    assert rc == _lib.EINVAL and b'too small' in msg
    rc, msg = call(ws_bytes=75 * 8 - 8)
    assert rc == _lib.EINVAL and b'workspace' in msg
    assert call(pair_iou=0.0)[0] == _lib.EINVAL and call(pair_iou=1.5)[0] == _lib.EINVAL and call(pair_iou=float('nan'))[0] == _lib.EINVAL
    assert call(n_pred=-1, ws_bytes=4096)[0] == _lib.EINVAL and call(n_true=-1, ws_bytes=4096)[0] == _lib.EINVAL
    assert call(pl=FAKE + 4)[0] == _lib.EINVAL and call(hit=FAKE + 1)[0] == _lib.EINVAL
