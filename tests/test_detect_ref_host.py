"""CPU-only proofs for the direct tests of csrc/detect.hip: tests/detect_ref.py is the reference's decode (tests/golden/decode.npz, the
reference's own outputs) and the eager tensor expressions of Detect.compute_outputs; every case of tests/detect_cases.py contains what it
says; oracle/nms_ref.c and the numpy restatements of oracle/nms_ref.py agree on every NMS case.

det_outputs: tests/golden/outputs.npz holds logits and final outputs but not the NMS rows between them, so `det_outputs` is checked against
the eager torch expressions (yolo_head.py:335-345 with hierarchical_scores as in-place child *= parent) on the det_outputs cases, NaN rows
included: that pins the NaN policy to torch.max.
"""
import os

import numpy as np
import pytest
import torch

import detect_cases as dc
import detect_ref as ref
from oracle import nms_ref

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


# ------------------------------------------------------------------------------------------ decode
def test_decode_reproduces_the_reference_golden():
    g = np.load(os.path.join(GOLDEN, 'decode.npz'))
    strides = [8.0, 16.0, 32.0]
    for tag in ('default', 'odd'):
        for l in range(3):
            det, want = g[f'{tag}_det_{l}'], g[f'{tag}_pred_{l}']
            B, na, ny, nx, no = det.shape
            got = ref.decode(det, dc.ANCHORS_P5[l], strides[l], l)
            np.testing.assert_allclose(got[..., :no], want.reshape(B, -1, no), rtol=2e-6, atol=1e-5)
            assert (got[..., no] == l).all()


def test_decode_special_values():
    x = dc.SWEEP.reshape(1, 1, 1, 1, -1)
    out = ref.decode(x, [3.0, 5.0], 8.0, 2)[0, 0]
    s = ref.sigmoid(dc.SWEEP)
    assert np.isnan(s[-1]) and np.isnan(out[-2]) and np.isfinite(s[:-1]).all() and out[-1] == 2
    assert s[list(dc.SWEEP).index(np.float32(-1e4))] == 0 and s[list(dc.SWEEP).index(-np.inf)] == 0 and s[list(dc.SWEEP).index(np.inf)] == 1
    assert ((s[:-1] >= 0) & (s[:-1] <= 1)).all()
    assert out[0] == (2 * 0.5 - 0.5 + 0) * 8.0 and out[1] == 4.0 and out[4] == s[4]


def test_decode_bound_stays_below_the_asserted_tolerance():
    """the reporting bound and the asserted 1e-4 cannot cross: (2 |x| + 6) 2^-24 <= 1e-4 for every finite sweep value up to |x| = 100
    (1.23e-5 there).  The two remaining finite magnitudes, 1e4 and 3e38, are beyond |x| = 836, where the formula itself passes 1e-4; there
    the power 2^(-x log2 e) is below 2^-149 or above 2^128 whatever the rounding of its argument, so the fp32 expression gives exactly 0 or 1
    and the reference is exactly 0 or 1 as well: no error for the bound to describe."""
    finite = dc.SWEEP[np.isfinite(dc.SWEEP)]
    near = finite[np.abs(finite) <= 100]
    far = finite[np.abs(finite) > 100]
    assert len(near) == 24 and len(far) == 4 and ref.decode_bound(near).max() <= 1e-4 and ref.decode_bound(near).max() < 1.3e-5
    assert (np.abs(far) * np.log2(np.e) > 150).all()
    s64, s32 = ref.sigmoid(far), ref.sigmoid(far, np.float32)
    assert np.array_equal(s64, (far > 0).astype(np.float64)) and np.array_equal(s32, (far > 0).astype(np.float32))


def test_sweep_is_the_listed_set():
    want = [0, 1e-30, 1e-3, 1, 20, 80, 87, 87.5, 88, 88.7, 89, 100, 1e4, 3e38, np.inf]
    for v in want:
        for sgn in (1.0, -1.0):
            hit = (dc.SWEEP == np.float32(sgn * v)) & (np.signbit(dc.SWEEP) == (sgn < 0))
            assert hit.sum() == 1, (v, sgn)
    assert np.isnan(dc.SWEEP).sum() == 1 and len(dc.SWEEP) == 2 * len(want) + 1


@pytest.mark.parametrize('name', list(dc.DECODE_LAYOUTS))
def test_decode_layouts_take_the_paths_they_are_listed_for(name):
    B, na, ny, nx, no, pitch = dc.DECODE_LAYOUTS[name]
    assert pitch >= na * no and pitch % 4 == 0 and pitch <= 64 and 1 <= na <= 8 and no >= 5
    want = 'tiled first branch' if no + 1 <= 16 else 'tiled second branch'
    assert dc.decode_path(name, 'pixel') == want
    assert dc.decode_path(name, 'contig') == 'per-candidate' and dc.decode_path(name, 'permuted') == 'per-candidate'
    # the sweep reaches every (anchor, column) with every value once there are at least 31 pixels
    v = dc.decode_values(name, 'sweep')
    if B * ny * nx >= len(dc.SWEEP):
        for a in range(na):
            for o in range(no):
                seen = v[:, a, :, :, o].ravel()
                assert np.isnan(seen).any() and len(np.unique(seen[~np.isnan(seen)].view(np.uint32))) == len(dc.SWEEP) - 1, (a, o)
    r = dc.decode_values(name, 'randn')
    assert np.isfinite(r).all() and 3.0 < r.std() < 5.0 or r.size < 100


def test_decode_branch_and_tile_statements():
    L = dc.DECODE_LAYOUTS
    assert L['d'][4] + 1 == 16 and L['e'][4] + 1 == 17 and L['e'][5] == L['e'][1] * L['e'][4] and L['f'][5] == 64 and L['b'][4] == 5
    assert L['c'][5] % 4 == 0 and L['c'][5] % 8 != 0
    B, na, ny, nx, no, pitch = L['j']
    assert -(-dc.DEC_TP // (ny * nx)) + 1 >= 8 and 128 // (ny * nx) == 8                # a 128-pixel tile covers 8 whole images and part of a ninth
    assert L['k'][2] * L['k'][3] == 1 and L['l'][0] * L['l'][2] * L['l'][3] < 16
    for name in dc.DECODE_FALLBACKS:
        assert dc.decode_path(name, 'pixel') == 'per-candidate'
    assert dc.DECODE_FALLBACKS['pitch68'][5] > 64 and dc.DECODE_FALLBACKS['pitch27'][5] % 4 != 0
    assert dc.DECODE_FALLBACKS['misaligned'] == L['a']
    B, na, ny, nx, no, pitch = dc.DECODE_LARGE['tiled']
    assert dc.decode_path('tiled', 'pixel') == 'tiled first branch' and B * ny * nx > dc.DEC_TILE_GRID * dc.DEC_TP
    B, na, ny, nx, no, pitch = dc.DECODE_LARGE['percand']
    assert dc.decode_path('percand', 'contig') == 'per-candidate' and B * na * ny * nx > dc.DEC_CAND_GRID
    strides = {dc.decode_setup(n)[2] for n in dc.DECODE_LAYOUTS}
    assert strides == {8.0, 16.0, 32.0, 64.0}
    assert any(any(v != int(v) for v in dc.decode_setup(n)[1]) for n in dc.DECODE_LAYOUTS)


def test_cpu_fp32_sigmoid_in_units_of_decode_bound():
    """the bracketed CPU column of the GPU file's table: the kernels' expression rounded in fp32 by numpy, per fill"""
    for fill in dc.FILLS:
        worst, med = 0.0, []
        for name in dc.DECODE_LAYOUTS:
            spec, anc, st, lvl = dc.decode_setup(name)
            det = dc.decode_values(name, fill)
            got = ref.decode(det, anc, st, lvl, dtype=np.float32)
            r = ref.decode_error_in_units(got, det, anc, st)
            if len(r):
                worst = max(worst, float(r.max()))
                med.append(float(np.median(r)))
        print(f'DETFIG cpu fp32 | {fill} | worst {worst:.3f} median {np.median(med):.3f}')
        assert worst <= 1.0                           # numpy's exp and division are correctly rounded or close to it: inside the 1-ulp model


# ------------------------------------------------------------------------------------------ NMS
def second_opinion(c):
    """oracle C against the numpy restatement; returns the oracle's result"""
    e = ref.nms_expected(c['preds'], c['nc'], c['conf'], c['iou'], c['max_det'], c['min_wh'], c['class_aware'])
    if c['class_aware']:
        preds = c['preds'][..., :5 + c['nc']]
        with np.errstate(invalid='ignore', over='ignore'):
            out = nms_ref.non_max_suppression_numpy(preds, c['conf'], c['iou'], max_det=c['max_det'])
        for b, det in enumerate(out):
            n = e['n_keep'][b]
            assert len(det) == n
            assert np.array_equal(det[:, :4], e['boxes'][b]) and np.array_equal(det[:, 4], e['conf'][b])
            assert np.array_equal(det[:, 5].astype(np.int32), e['cls'][b, :n])
    else:
        with np.errstate(invalid='ignore', over='ignore'):
            out = nms_ref.nms_per_image_numpy(c['preds'], c['nc'], c['conf'], c['iou'], c['max_det'], c['min_wh'])
        for b, o in enumerate(out):
            n = e['n_keep'][b]
            assert np.array_equal(o['index'], e['keep'][b, :n]), b
            assert np.array_equal(o['boxes'], e['boxes'][b], equal_nan=True) and np.array_equal(o['scores'], e['scores'][b], equal_nan=True)
            assert np.array_equal(o['extra'], e['extra'][b], equal_nan=True)
    assert (e['keep'][np.arange(c['max_det'])[None] >= e['n_keep'][:, None]] == -1).all()
    return e


@pytest.mark.parametrize('min_wh', dc.FILTER_MIN_WH)
def test_filter_edges_shares(min_wh):
    c = dc.nms_filter_edges(min_wh)
    e = second_opinion(c)
    p = c['preds']
    assert (p[..., 0:2] == np.round(p[..., 0:2])).all() and (p[..., 4] > c['conf']).all()
    m = np.float32(min_wh)
    for b in range(p.shape[0]):
        small = (p[b, :, 2] < m) | (p[b, :, 3] < m)
        edge = ~small & ((p[b, :, 2] == m) | (p[b, :, 3] == m))
        print(f'min_wh {min_wh} image {b}: rejected by size {small.mean():.3f}, on the edge and passing {edge.mean():.3f}, kept {e["n_keep"][b]}')
        assert small.mean() >= 0.30 and edge.mean() >= 0.30
        kept = np.zeros(p.shape[1], bool)
        kept[e['keep'][b, :e['n_keep'][b]]] = True
        assert not kept[small].any() and kept[edge].sum() > 0.5 * edge.sum()         # `>` for `>=` would drop every edge row


@pytest.mark.parametrize('conf', dc.STRICT_CONF)
def test_strict_conf_thirds(conf):
    c = dc.nms_strict_conf(conf)
    e = second_opinion(c)
    s = c['preds'][0, :, 4]
    cf = np.float32(conf)
    assert (s == cf).sum() == 1000 and (s > cf).sum() == 1000 and (s < cf).sum() == 1000
    assert len(np.unique(s)) == 3
    kept = e['keep'][0, :e['n_keep'][0]]
    assert len(kept) > 500 and (s[kept] > cf).all()                                   # `>=` would let the rows equal to conf in
    assert (np.diff(kept) > 0).all()                                                   # all kept scores are equal: ties go by row


@pytest.mark.parametrize('kind', dc.IOU_SETS)
@pytest.mark.parametrize('iou', [0.0, 1.0])
def test_iou_threshold_ends(kind, iou):
    c = dc.nms_iou(kind, iou)
    e = second_opinion(c)
    n = e['n_keep'][0]
    if iou == 1.0:
        assert n == c['preds'].shape[1]                                                # nothing exceeds 1: everything stays
    elif kind == 'duplicates':
        assert n <= c['preds'].shape[1] // 2
    else:
        assert 0 < n < c['preds'].shape[1] // 4


@pytest.mark.parametrize('M', dc.SURVIVORS)
def test_survivor_counts(M):
    for md in dc.survivor_max_dets(M):
        c = dc.nms_survivors(M, md)
        p = c['preds'][0]
        assert p.shape[0] == M + 500 and (p[:, 4] > c['conf']).sum() == M
        if md == max(M, 1):
            e = second_opinion(c)
            assert e['n_keep'][0] >= M / 2 and e['n_keep'][0] <= M
            low = np.nonzero(p[:, 4] <= c['conf'])[0]
            assert len(low) == 500 and (M == 0 or (low.min() < M // 2 + 250 and low.max() > M // 2))      # interleaved
            full = e
        else:
            e = ref.nms_expected(c['preds'], c['nc'], c['conf'], c['iou'], md)
            n = min(md, full['n_keep'][0])
            assert e['n_keep'][0] == n and np.array_equal(e['keep'][0, :n], full['keep'][0, :n])
    assert dc.kept_list(4096) == 'LDS kept list' and dc.kept_list(4097) == 'workspace kept list'


def test_mixed_batch_and_empty_rows():
    counts = dc.mixed_counts()
    assert len(counts) == dc.MIXED_B and set(dc.SURVIVORS) <= set(counts) and counts.count(-1) == 2
    c = dc.nms_mixed_batch()
    p = c['preds']
    assert p.shape[:2] == (64, 8693)
    for b, m in enumerate(counts):
        assert (p[b, :, 4] > c['conf']).sum() == max(m, 0)
    e = ref.nms_expected(c['preds'], c['nc'], c['conf'], c['iou'], c['max_det'])
    assert [int(v) for v in e['n_keep']] == [min(300, int(v)) if m > 600 else int(v) for v, m in zip(e['n_keep'], counts)]
    second_opinion(c)
    z = dc.nms_empty_rows()
    e = ref.nms_expected(z['preds'], z['nc'], z['conf'], z['iou'], z['max_det'])
    assert z['preds'].shape == (3, 0, 7) and (e['n_keep'] == 0).all() and (e['keep'] == -1).all()


def test_precut_statements():
    c, iso = dc.nms_precut()
    p = c['preds'][0]
    assert p.shape[0] == 33000 and len(iso) == dc.PRECUT_ISOLATED and (p[:, 4] == np.float32(0.1)).sum() == 1200
    score, _ = ref.best_class(p, c['nc'])
    passing = (p[:, 4] > np.float32(c['conf'])) & (score > np.float32(c['conf']))
    assert passing.sum() > dc.PRECUT and passing[iso].all()                                            # (i)
    order = np.argsort(-np.where(passing, score, -1), kind='stable')
    rank = np.empty(len(p), np.int64)
    rank[order] = np.arange(len(p))
    assert rank[iso].min() >= dc.PRECUT                                                                # (ii)
    e = second_opinion(c)
    kept = e['keep'][0, :e['n_keep'][0]]
    assert e['n_keep'][0] < c['max_det'] and not np.isin(iso, kept).any()                              # (iii), and the cut took them
    c2, iso2 = dc.nms_precut(below=True)
    assert np.array_equal(iso, iso2)
    p2 = c2['preds'][0]
    score2, _ = ref.best_class(p2, c2['nc'])
    passing2 = (p2[:, 4] > np.float32(c2['conf'])) & (score2 > np.float32(c2['conf']))
    assert passing2.sum() < dc.PRECUT and passing.sum() - passing2.sum() == 1500
    e2 = second_opinion(c2)
    kept2 = e2['keep'][0, :e2['n_keep'][0]]
    assert e2['n_keep'][0] < c2['max_det'] and np.isin(iso, kept2).all()                               # (iv)
    print(f'pre-cut: {passing.sum()} pass, isolated rank from {rank[iso].min()}, kept {len(kept)} with the cut, {len(kept2)} below it')
    centre = p[passing & ~np.isin(np.arange(len(p)), iso)][:, :2]
    assert centre.min() >= 0 and centre.max() <= 60


def test_class_offsets_statements():
    c = dc.nms_class_offsets()
    e = second_opinion(c)
    p = c['preds']
    assert p.shape == (2, 1500, 86) and c['nc'] == 80
    for b in range(2):
        _, cls = ref.best_class(p[b], 80)
        assert set(cls) == set(range(80))
        kept = np.zeros(1500, bool)
        kept[e['keep'][b, :e['n_keep'][b]]] = True
        same = [(i, i + 1) for i in range(0, 1500, 4) if cls[i] == cls[i + 1]]
        diff = [(i, i + 1) for i in range(2, 1500, 4) if cls[i] != cls[i + 1]]
        assert len(same) > 300 and len(diff) > 300
        assert all(np.array_equal(p[b, i, :4], p[b, j, :4]) for i, j in same + diff)
        assert not any(kept[i] and kept[j] for i, j in same)                      # identical boxes of one class: never both
        assert sum(kept[i] and kept[j] for i, j in diff) > 100                    # of different classes: the offset separates them
        ties = [r for r in range(0, 1500, 5) if (p[b, r, 5:85] == np.float32(0.9)).sum() == 2]
        assert len(ties) > 200 and all(cls[r] == np.nonzero(p[b, r, 5:85] == np.float32(0.9))[0][0] for r in ties)
        assert cls.max() * 7680 == 606720


def test_nonfinite_rows_agree():
    c = dc.nms_nonfinite()
    e = second_opinion(c)                                                          # asserts that oracle C and numpy agree
    p = c['preds']
    bad = ~np.isfinite(p[..., :5])
    assert (bad.sum(-1) <= 1).all() and abs(bad.any(-1).sum() - 2 * 286) <= 2
    combos = {(int(np.nonzero(r)[0][0]), str(p[b, i, np.nonzero(r)[0][0]])) for b in range(2) for i, r in enumerate(bad[b]) if r.any()}
    assert len(combos) == 15
    kept_bad = sum(int(bad[b, e['keep'][b, :e['n_keep'][b]]].any(-1).sum()) for b in range(2))
    print(f'non-finite: kept {list(e["n_keep"])}, {kept_bad} non-finite rows among them')
    assert kept_bad > 0


@pytest.mark.parametrize('M', dc.SURVIVORS)
def test_xyxy_survivor_sets(M):
    b, s = dc.xyxy_survivors(M)
    assert b.shape == (M, 4) and s.shape == (M,)
    keep = nms_ref.nms_c(b, s, 0.45)
    assert np.array_equal(keep, nms_ref.nms_numpy(b, s, 0.45)) and len(keep) >= M / 2


# ------------------------------------------------------------------------------------------ det_outputs
def eager_outputs(scores, boxes, n_keep, pairs, conf, ml):
    """Detect.compute_outputs' tail per image, in torch on the CPU"""
    scores = torch.from_numpy(scores.copy())
    ob, os_, ol = [], [], []
    for b in range(scores.shape[0]):
        x = scores[b, :int(n_keep[b])]
        for c, p in pairs:
            x[:, c] *= x[:, p]
        ob.append(torch.from_numpy(boxes[b, :int(n_keep[b])]))
        if ml:
            os_.append(x.clone())
            ol.append(x > conf)
        elif len(x):
            obj = x[..., 0]
            cs, cl = x[..., 1:].max(1)
            os_.append(torch.where(cs > conf, cs, obj))
            ol.append(torch.where(cs > conf, cl + 1, -100))
    cat = (lambda v, e: torch.cat(v) if v else e)
    return scores, cat(ob, torch.zeros((0, 4))), cat(os_, torch.zeros(0)), cat(ol, torch.zeros(0, dtype=torch.int64))


@pytest.mark.parametrize('B,nc,tree,edge_empty', dc.OUT_CASES)
@pytest.mark.parametrize('ml', [False, True])
def test_det_outputs_is_the_eager_expression(B, nc, tree, edge_empty, ml):
    c = dc.det_outputs_case(B, nc, tree, edge_empty)
    got = ref.det_outputs(c['scores'], c['boxes'], c['n_keep'], c['pairs'], c['conf'], ml)
    sc, bx, s, l = eager_outputs(c['scores'], c['boxes'], c['n_keep'], c['pairs'], c['conf'], ml)
    total = int(c['n_keep'].sum())
    assert got['offsets'][-1] == total and np.array_equal(np.diff(got['offsets']), c['n_keep'])
    assert np.array_equal(got['scores_inplace'].view(np.uint32), sc.numpy().view(np.uint32))
    assert np.array_equal(got['boxes'], bx.numpy())
    assert np.array_equal(got['scores'], s.numpy(), equal_nan=True) and np.array_equal(got['labels'], l.numpy())
    n = c['n_keep']
    assert {0, 1, c['max_det']} <= set(int(v) for v in n) or B == 1
    assert (n[0] == 0 and n[-1] == 0) == bool(edge_empty)
    if B == 300:
        assert c['max_det'] == 12 and B > 256                                        # the prefix loop strides
    if not ml and nc > 1 and not tree and total:
        # case (b): a NaN in a later class column hides a finite score above conf: torch.max gives NaN, no hit, label -100
        rows = [(b, j) for b in range(B) for j in range(int(n[b])) if j % 16 == 9]
        assert rows
        for b, j in rows:
            k = got['offsets'][b] + j
            assert got['labels'][k] == -100 and got['scores'][k] == c['scores'][b, j, 0] and c['scores'][b, j, 1] > c['conf']


# ------------------------------------------------------------------------------------------ det_grad_pack
def test_grad_pack_rounding_and_shapes():
    v = dc.PACK_SPECIALS
    r = ref.q_bf16(v)
    want = {1.00390625: 1.0, 1.01171875: 1.015625, -1.00390625: -1.0, -1.01171875: -1.015625, 1.00390637: 1.0078125, 1.00390613: 1.0}
    for a, b in want.items():
        assert r[list(v).index(np.float32(a))] == np.float32(b), a
    assert np.isnan(r[2]) and r[3] == np.inf and r[4] == -np.inf and np.signbit(r[1]) and r[1] == 0
    assert r[list(v).index(np.float32(3.4028235e38))] == np.inf and r[list(v).index(np.float32(3.3895314e38))] == np.float32(3.3895314e38)
    assert np.array_equal(r.view(np.uint32) & 0xffff, np.zeros(len(v), np.uint32)) or np.isnan(r).any()
    t = torch.from_numpy(v).to(torch.bfloat16).float().numpy()                      # ATen's conversion is the same rounding
    assert np.array_equal(t[~np.isnan(v)].view(np.uint32), r[~np.isnan(v)].view(np.uint32))
    (shape, ldo) = dc.PACK_SHAPES[-1]
    B, na, ny, nx, no = shape
    assert B * ny * nx * ldo == dc.PACK_GRID + 1 and ldo >= na * no
    g = dc.grad_pack_values((2, 3, 7, 9, 13))
    out = ref.grad_pack(g, 3, 13, 48, 'f32')
    assert out.shape == (2, 7, 9, 48) and (out[..., 39:] == 0).all() and not np.signbit(out[..., 39:]).any()
    assert np.array_equal(out[1, 2, 3, 13 * 2 + 5].view(np.uint32), g[1, 2, 2, 3, 5].view(np.uint32))
    assert np.isnan(g).any() and np.isinf(g).any()
