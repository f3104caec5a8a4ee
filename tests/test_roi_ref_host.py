"""CPU only.  Pins tests/roi_ref.py (the float64 restatement the direct tests of csrc/roi.hip compare with) to oracle/mask_ref.roi_align under
torch float64 autograd at 1e-12 of the tensor's largest value, proves that every case of tests/roi_cases.py holds the classes it is named
for (in fp32, as the kernel classifies, and in float64), that every sample stays KINK_MARGIN coordinate bounds away from a validity threshold
(the dyadic case: fp32 and float64 coordinates are equal), that the stored rois miss the closed-form footprint, that the footprint rule read
from roi.hip's text keeps every table write inside the footprint, and that the comparers reject each of a list of wrong evaluations."""
import os
import re

import numpy as np
import pytest
import torch

import roi_cases as rc
import roi_ref as ref
from oracle import mask_ref

PIN = 1e-12
SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hd_yolo_amd', 'csrc', 'roi.hip')).read()


def pin(got, want, what):
    got, want = np.asarray(got, np.float64), want.detach().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max() if got.size else 0.0
    assert err <= PIN * max(np.abs(want).max() if want.size else 0.0, 1e-300), f'{what}: {err:.3g}'


def all_cases():
    for c in rc.GRID:
        yield rc.case_id(c), rc.grid_case(c)
    for dt in rc.DTYPES:
        for name in rc.SPECIAL:
            yield f'{name}-{dt}', rc.special_case(name, dt)
        for m in rc.MISSES:
            yield f'{m[0]}-{dt}', rc.miss_case(m, dt)


def classify(c, rule='samples', rois=None):
    return rc.classify(c['rois'] if rois is None else rois, c['scale'], c['P'], c['S'], c['aligned'], c['B'], c['H'], c['W'], rule)


# ------------------------------------------------------------------------------------------ the kernel's text
def test_constants_are_those_of_the_kernel_source():
    for name, val in (('FT', rc.FT), ('CB', rc.CB), ('PM', rc.PM)):
        m = re.search(rf'constexpr int {name} = (\d+);', SRC)
        assert m and int(m.group(1)) == val, name
    assert 'const bool tiled = fh <= FT && fw <= FT && P <= PM;' in SRC
    assert re.search(r'dim3 grid\(R, \(C \+ CB - 1\) / CB\)', SRC)
    assert 'hdy_note_dispatch("roi_align_bwd")' in SRC


def source_rule():
    """which footprint rule the tiled kernel's text holds: the closed form of the top sample, or the range of the samples themselves"""
    closed = '((float)P - 0.5f / (float)S)' in SRC
    samples = 'atomicMin(&fpt[' in SRC and 'atomicMax(&fpt[' in SRC and SRC.count('axis_coord(') >= 3
    assert closed != samples, 'roi.hip: footprint rule not recognised'
    return 'closed' if closed else 'samples'


def test_no_table_write_leaves_the_footprint_under_the_rule_of_the_source():
    """the fp32 classification under the rule roi.hip has: no valid sample index outside the footprint, on any case or stored roi"""
    rule = source_rule()
    for name, c in all_cases():
        k = classify(c, rule)
        assert not k['escape_y'].any() and not k['escape_x'].any(), f'{name}: a sample index outside the {rule} footprint (rois {np.nonzero(k["escape_y"] | k["escape_x"])[0]})'


@pytest.mark.parametrize('m', rc.MISSES, ids=[m[0] for m in rc.MISSES])
def test_stored_rois_miss_the_closed_form_footprint(m):
    name, P, S, aligned, scale, H, W, roi = m
    axis, want_n = rc.MISS_SEARCH[name]
    c = rc.miss_case(m)
    k, new = classify(c, 'closed'), classify(c, 'samples')
    assert k['escape_' + axis][0] and not k['escape_' + axis][1] and not k['escape_' + ('x' if axis == 'y' else 'y')].any()
    assert not new['escape_y'].any() and not new['escape_x'].any()
    n_closed, n_true = k['fh' if axis == 'y' else 'fw'][0], new['fh' if axis == 'y' else 'fw'][0]
    assert n_true == n_closed + 1 and k['tiled'][0]
    g = k['geom']
    v = g[axis + 's'][0, -1]                                  # the top sample lies on the integer: the stray weight is 0
    assert v == np.rint(v) and ref.axis_sample(g[axis + 's'][:1], H)[4][0, -1] == 0
    if want_n:
        assert n_closed == rc.FT and P == rc.PM and new['scatter'][0] and not new['tiled'][0], 'a true footprint of FT + 1 takes the scatter path'
    assert new['tiled'][0] == (n_true <= rc.FT)
    assert new['tiled'][1] == k['tiled'][1]                   # the ordinary roi beside it is classified as before


def test_the_seeded_search_finds_such_rois():
    for name, P, S, aligned, scale, H, W, roi in rc.MISSES[:1] + rc.MISSES[4:5]:
        axis, want_n = rc.MISS_SEARCH[name]
        found = rc.search_misses(P, S, aligned, scale, H, W, axis, 0, want_n=want_n, tries=300)
        assert len(found) >= 1, name


# ------------------------------------------------------------------------------------------ what the cases contain
def sample_tables(c, dtype):
    g = ref.geometry(c['rois'], c['scale'], c['P'], c['S'], c['aligned'], dtype)
    return g, ref.axis_sample(g['ys'], c['H']), ref.axis_sample(g['xs'], c['W'])


@pytest.mark.parametrize('case', rc.GRID, ids=rc.case_id)
def test_grid_case_holds_its_classes(case):
    dt, C, P, S, aligned, kind, scale = case
    c = rc.grid_case(case)
    H, W, cls = c['H'], c['W'], np.array(c['cls'])
    assert H <= 48 and W <= 48 and c['B'] <= 3 and len(c['rois']) <= 64
    assert ref.kink_distance(c['rois'], scale, P, S, aligned, H, W) >= ref.KINK_MARGIN
    k32 = classify(c)
    for dtype in (np.float32, np.float64):
        g, (oky, y0, y1, _, _), (okx, x0, x1, _, _) = sample_tables(c, dtype)
        of = lambda name: np.nonzero(cls == name)[0]                                     # noqa: E731
        assert UNNAMED not in g['b'] and set(g['b']) <= {-1, 0, 2, 3}
        if kind in ('small', 'mixed'):
            r = of('overlap')
            assert len(r) == 8 and all(oky[i].all() and okx[i].all() and y0[i].min() <= 20 <= y1[i].max() and x0[i].min() <= 20 <= x1[i].max() for i in r)
            assert all(g['b'][i] == 0 for i in r)
            for i in of('interior'):
                assert oky[i].all() and okx[i].all() and 1 <= y0[i].min() and y1[i].max() <= H - 2 and x1[i].max() - x0[i].min() < 12
            raw = c['rois'].astype(np.float64)
            for i in of('narrow'):
                assert 0 < (raw[i, 3] - raw[i, 1]) * scale < 1 and 0 < (raw[i, 4] - raw[i, 2]) * scale < 1
                assert np.allclose(g['bin_w'][i] * P, (raw[i, 3] - raw[i, 1]) * scale if aligned else 1.0, atol=1e-5)
            for i in of('zero'):
                assert raw[i, 3] == raw[i, 1] and raw[i, 4] == raw[i, 2] and g['bin_w'][i] == (0.0 if aligned else dtype(1.0) / dtype(P))
            xs, ys = g['xs'], g['ys']
            assert any(((xs[i] >= -1) & (xs[i] < 0)).any() for i in of('left')) and any(((ys[i] >= -1) & (ys[i] < 0)).any() for i in of('top'))
            assert any(((xs[i] > W - 1) & (xs[i] <= W)).any() for i in of('right')) and any(((ys[i] > H - 1) & (ys[i] <= H)).any() for i in of('bottom'))
            if P * S > 2:                                                                      # and samples beyond the thresholds
                assert any((xs[i] < -1).any() and okx[i].any() for i in of('left')) and any((ys[i] > H).any() and oky[i].any() for i in of('bottom'))
            assert len(of('outside')) == 2 and all(not (oky[i][:, None] & okx[i][None]).any() for i in of('outside'))
            assert not okx[of('outside')[0]].any() and not oky[of('outside')[1]].any()
            assert g['b'][of('img-1')[0]] == -1 and g['b'][of('imgB')[0]] == c['B']
        if kind in ('large', 'mixed'):
            i = of('whole')[0]
            assert np.array_equal(c['rois'][i], np.array([0, 0, 0, W / scale, H / scale], np.float32)) and oky[i].all() and okx[i].all()
            if P * S >= 28:
                assert y0[i].min() <= 1 and y1[i].max() >= H - 2 and x0[i].min() <= 1 and x1[i].max() >= W - 2
        dx, dy = ref.coord_error(c['rois'], scale, P, aligned)
        for name, (fh, fw) in rc.FP_CLASSES.items():
            for i in of(name):
                assert (y1[i].max() - y0[i].min() + 1, x1[i].max() - x0[i].min() + 1) == (fh, fw), (name, dtype)
                for v, d in ((g['ys'][i], dy[i]), (g['xs'][i], dx[i])):                       # away from a classification flip
                    assert min(abs(v[0] - np.rint(v[0])), abs(v[-1] - np.rint(v[-1]))) > 0.2 > ref.KINK_MARGIN * d
                assert (k32['fh'][i], k32['fw'][i]) == (fh, fw)
    UNN = UNNAMED
    assert UNN not in c['rois'][:, 0]
    live = k32['live']
    assert not live[cls == 'outside'].any() and not live[cls == 'img-1'].any() and not live[cls == 'imgB'].any()
    if P > rc.PM or kind == 'large':
        assert k32['scatter'][live].all() and not k32['tiled'].any()
    elif kind == 'small':
        assert k32['tiled'][live].all() and not k32['scatter'].any()
    else:
        assert k32['tiled'].sum() >= 20 and k32['scatter'].sum() >= 5 and k32['tiled'][cls == 'fp24x24'].all()
        assert k32['scatter'][np.isin(cls, ('fp24x25', 'fp25x24', 'fp30x30', 'whole'))].all()


UNNAMED = rc.UNNAMED


def test_grid_covers_the_parameter_values():
    for dt in rc.DTYPES:
        rows = [c for c in rc.GRID if c[0] == dt]
        assert {c[1] for c in rows} == set(rc.CHANNELS[dt]) and {c[2] for c in rows} == {1, 7, 14, 16, 17, 28}
        assert {c[3] for c in rows} == {1, 2, 3, 4} and {c[4] for c in rows} == {False, True}
        for P in (1, 7, 14, 16):                                                              # both backward paths
            assert {'small', 'large'} <= {c[5] for c in rows if c[2] == P} or 'mixed' in {c[5] for c in rows if c[2] == P}
        for S in (1, 2, 3, 4):
            kinds = {c[5] for c in rows if c[3] == S and c[2] <= rc.PM}
            assert kinds & {'small', 'mixed'} and kinds & {'large', 'mixed'}
    assert len(rc.GRID) == 40
    assert rc.CHANNELS['f32'] == (4, 36, 72) and rc.CHANNELS['bf16'] == (8, 40, 72)          # a partial block; two, the last partial; three


@pytest.mark.parametrize('dt', rc.DTYPES)
def test_special_cases(dt):
    c = rc.special_case('dyadic', dt)
    g32, g64 = (ref.geometry(c['rois'], c['scale'], c['P'], c['S'], c['aligned'], t) for t in (np.float32, np.float64))
    for k in ('xs', 'ys', 'bin_w', 'bin_h'):
        assert np.array_equal(g32[k].astype(np.float64), g64[k]), k
    assert (g64['ys'] == -1).any() and (g64['ys'] == c['H']).any() and (g64['xs'] == -1).any() and (g64['xs'] == c['W']).any()
    assert (g64['ys'] < -1).any() and (g64['ys'] > c['H']).any()
    assert np.array_equal(g64['ys'] * 8, np.rint(g64['ys'] * 8))
    for name in ('h1', 'w1'):
        c = rc.special_case(name, dt)
        assert (c['H'], c['W']) == ((1, 20) if name == 'h1' else (20, 1))
        assert ref.kink_distance(c['rois'], c['scale'], c['P'], c['S'], c['aligned'], c['H'], c['W']) >= ref.KINK_MARGIN
        k = classify(c)
        assert k['live'].all() and k['tiled'].all() and ((k['fh'] if name == 'h1' else k['fw']) == 1).all()
        g, (oky, *_), (okx, *_) = sample_tables(c, np.float64)
        ok = oky if name == 'h1' else okx
        assert ok[0].all() and ok[1].all() and not ok[2].all() and ok[2].any()


@pytest.mark.parametrize('case', rc.NONFINITE_BWD, ids=rc.case_id)
def test_nonfinite_gradient_bins_are_away_from_an_integer(case):
    """the reference's pattern (the neighbours of the bin's samples) must not hinge on a rounding"""
    c = rc.grid_case(case)
    d, which = rc.plant_nonfinite_dout(c)
    assert (~np.isfinite(d)).sum() == 2 and which.sum() == 2
    g = ref.geometry(c['rois'], c['scale'], c['P'], c['S'], c['aligned'])
    dx, dy = ref.coord_error(c['rois'], c['scale'], c['P'], c['aligned'])
    k = classify(c)
    for (name, (p, qq), ch, val), path in zip(rc.NONFINITE_AT, ('tiled', 'scatter')):
        r = c['cls'].index(name)
        assert k[path][r]
        for v, e, b in ((g['ys'][r], dy[r], p), (g['xs'][r], dx[r], qq)):
            s = v[b * c['S']:(b + 1) * c['S']]
            assert (np.abs(s - np.rint(s)) > ref.KINK_MARGIN * e).all()
    out = ref.roi_align_bwd(d, (c['B'], c['H'], c['W'], c['C']), c['rois'], c['scale'], c['S'], c['aligned'])
    may = ref.footprint_mask(out.shape, c['rois'], c['scale'], c['P'], c['S'], c['aligned'], which)
    bad = ~np.isfinite(out)
    assert bad.any() and not (bad & ~may).any() and bad.sum() < may.sum()
    assert set(np.nonzero(bad)[3]) == {1, 2} and np.isfinite(out[UNNAMED]).all()


# ------------------------------------------------------------------------------------------ pins
def torch_roi(c, feat=None):
    f = torch.from_numpy(np.asarray(c['feat'] if feat is None else feat, np.float64)).permute(0, 3, 1, 2).clone().requires_grad_(True)
    rois = torch.from_numpy(c['rois']).double()
    live = (rois[:, 0] >= 0) & (rois[:, 0] < c['B'])
    out = torch.zeros((len(rois), c['C'], c['P'], c['P']), dtype=torch.float64)
    out[live] = mask_ref.roi_align(f, rois[live], c['P'], float(np.float32(c['scale'])), c['S'], c['aligned'])
    out.backward(torch.from_numpy(c['dout']).double().permute(0, 3, 1, 2))
    return out.permute(0, 2, 3, 1), f.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize('case', [c for c in rc.GRID if c[0] == 'f32'], ids=rc.case_id)
def test_restatement_equals_the_oracle_under_float64_autograd(case):
    c = rc.grid_case(case)
    out, grad = torch_roi(c)
    pin(ref.roi_align_fwd(c['feat'], c['rois'], c['scale'], c['P'], c['S'], c['aligned']), out, 'forward')
    shape = (c['B'], c['H'], c['W'], c['C'])
    pin(ref.roi_align_bwd(c['dout'], shape, c['rois'], c['scale'], c['S'], c['aligned']), grad, 'backward')
    into = ref.roi_align_bwd(c['dout'], shape, c['rois'], c['scale'], c['S'], c['aligned'], into=c['into'])
    pin(into, grad + torch.from_numpy(c['into']).double(), 'backward into')
    assert np.array_equal(into[UNNAMED], c['into'][UNNAMED].astype(np.float64)) and not grad[UNNAMED].any()


@pytest.mark.parametrize('name', rc.SPECIAL)
def test_special_cases_equal_the_oracle(name):
    c = rc.special_case(name, 'f32')
    out, grad = torch_roi(c)
    pin(ref.roi_align_fwd(c['feat'], c['rois'], c['scale'], c['P'], c['S'], c['aligned']), out, 'forward')
    pin(ref.roi_align_bwd(c['dout'], (c['B'], c['H'], c['W'], c['C']), c['rois'], c['scale'], c['S'], c['aligned']), grad, 'backward')


def test_nonfinite_features_reach_the_bins_of_their_valid_samples():
    c = rc.special_case('dyadic', 'f32')
    f = rc.plant_nonfinite_features(c)
    out, bound = ref.roi_align_fwd(f, c['rois'], c['scale'], c['P'], c['S'], c['aligned'], with_bound=True)
    clean = ref.roi_align_fwd(c['feat'], c['rois'], c['scale'], c['P'], c['S'], c['aligned'])
    bad = ~np.isfinite(out)
    assert bad.any() and np.isinf(out).any() and np.isnan(out).any() and np.isfinite(bound[~bad]).all()
    assert not bad[1].any() and set(np.nonzero(bad)[3]) == {1, 2}                # image 1 holds none; the channels of the two plants
    assert np.array_equal(out[~bad], clean[~bad])
    assert np.isnan(out[0, :, :, 1]).sum() == 4                                 # the bins with a sample in rows and columns (4, 6)


# ------------------------------------------------------------------------------------------ multi-level
@pytest.mark.parametrize('nb,P', rc.LEVELS)
def test_levels_form_equals_the_per_level_assembly(nb, P):
    c = rc.levels_case(nb, P, 'f32')
    n = np.clip(c['n_keep'], 0, rc.MAX_DET)
    total = int(n.sum())
    assert (c['n_keep'] == 0).any() or nb == 1
    if nb >= 4:
        assert (c['n_keep'] < 0).any() and (c['n_keep'] > rc.MAX_DET).any()
    rows = [(b, j) for b in range(nb) for j in range(n[b])]
    lv = np.array([c['level'][r] for r in rows])
    for out_rows in (max(total - 2, 0), total, total + 2):
        out, bound, written = ref.roi_align_levels(c['feats'], c['scales'], c['boxes'], c['level'], c['n_keep'], out_rows, P, 2, False, 123.0)
        assert written == min(out_rows, total) and (out[written:] == 123.0).all() and out.shape[0] == out_rows
        for k in range(written):                                 # Detect.attach_masks' assembly: one single-level call per row
            b, j = rows[k]
            l = lv[k]
            if np.isfinite(l) and -1 < l < 2:
                want = ref.roi_align_fwd(c['feats'][int(l)], [[b, *c['boxes'][b, j]]], c['scales'][int(l)], P, 2, False)[0]
                assert np.array_equal(out[k], want)
            else:
                assert not out[k].any() and not bound[k].any()
    if nb >= 260:
        assert (~np.isfinite(lv)).any() and (lv == 7).any() and (lv == -0.5).any()
    for l, side in enumerate(rc.LEVEL_SIDES):
        rois = np.array([[b, *c['boxes'][b, j]] for b, j in rows], np.float32)
        assert ref.kink_distance(rois, c['scales'][l], P, 2, False, side, side) >= ref.KINK_MARGIN


# ------------------------------------------------------------------------------------------ the comparers bite
def mutant_fwd(c, mut, at=None):
    """a separable float64 evaluation of the forward with one deliberate mistake; pixels -1 and `size` exist and hold zeros"""
    aligned = c['aligned'] != (mut == 'aligned')
    P, S, H, W = c['P'], c['S'], c['H'], c['W']
    r = c['rois'].astype(np.float64)
    s, off = float(np.float32(c['scale'])), 0.5 if aligned else 0.0
    out = np.zeros((len(r), P, P, c['C']))
    for k in range(len(r)):
        b = int(r[k, 0])
        if not 0 <= b < c['B']:
            continue
        mats = []
        for lo, hi, size in ((2, 4, H), (1, 3, W)):
            o = r[k, lo] * s - off
            w = r[k, hi] * s - off - o
            if not aligned and mut != 'width':
                w = max(w, 1.0)
            M = np.zeros((P, size + 2))
            for j in range(P * S):
                v = o + (j // S) * (w / P) + (j % S + 0.5) * (w / P) / S
                if v < -1 or v > size or (mut == 'ge' and v >= size and lo == 2):
                    continue
                if mut != 'clamp0':
                    v = max(v, 0.0)
                i0 = int(np.floor(v))
                if i0 >= size - 1 and mut != 'selfinterp':
                    i0, v = size - 1, float(size - 1)
                M[j // S, i0 + 1] += 1 - (v - i0)
                M[j // S, i0 + 2] += v - i0
            mats.append(M[:, 1:size + 1])
        out[k] = np.einsum('ph,qw,hwc->pqc', mats[0], mats[1], c['feat'][b].astype(np.float64)) / (S * S)
    return out


def fwd_with_bound(c):
    out, bound = ref.roi_align_fwd(c['feat'], c['rois'], c['scale'], c['P'], c['S'], c['aligned'], with_bound=True)
    return out, ref.finish(bound, out, c['dt'] == 'bf16')


@pytest.mark.parametrize('dt', rc.DTYPES)
def test_comparer_rejects_wrong_forward_evaluations(dt):
    c = rc.grid_case((dt, 72, 14, 2, False, 'mixed', 0.0625))
    out, bound = fwd_with_bound(c)
    assert ref.check(mutant_fwd(c, None), out, bound, 'the unmutated evaluation') < 1e-3
    assert ref.check(out + 0.5 * bound, out, bound) < 0.51 and ref.check(out - 0.5 * bound, out, bound) < 0.51
    for mut in ('aligned', 'clamp0', 'selfinterp', 'width'):
        with pytest.raises(AssertionError):
            ref.check(mutant_fwd(c, mut), out, bound, mut)
    r = c['cls'].index('interior')
    wrong = out.copy()
    wrong[r, 3, 5] *= c['S'] ** 2                                # 1 / S^2 missing in one bin
    with pytest.raises(AssertionError):
        ref.check(wrong, out, bound)
    wrong = out.copy()
    wrong[..., 32:64] = 0                                         # one 32-channel block zeroed
    with pytest.raises(AssertionError):
        ref.check(wrong, out, bound)
    wrong = out.copy()
    wrong[r, 3, 5, 7] += 2 * bound[r, 3, 5, 7]
    with pytest.raises(AssertionError):
        ref.check(wrong, out, bound)
    d = rc.special_case('dyadic', dt)                             # a sample exactly on `size` tested with >= instead of >
    out, bound = fwd_with_bound(d)
    assert ref.check(mutant_fwd(d, None), out, bound) < 1e-3
    with pytest.raises(AssertionError):
        ref.check(mutant_fwd(d, 'ge'), out, bound, 'ge')


@pytest.mark.parametrize('kind', ['small', 'large'])
def test_comparer_rejects_a_dropped_footprint_row(kind):
    c = rc.grid_case(('f32', 36, 14, 2, False, kind, 0.125))
    shape = (c['B'], c['H'], c['W'], c['C'])
    tiled = classify(c)['tiled']
    for into in (None, c['into']):
        g, bound = ref.roi_align_bwd(c['dout'], shape, c['rois'], c['scale'], c['S'], c['aligned'], into=into, with_bound=True, tiled=tiled)
        r = c['cls'].index('interior' if kind == 'small' else 'fp30x30')
        one = ref.roi_align_bwd(c['dout'][r:r + 1], shape, c['rois'][r:r + 1], c['scale'], c['S'], c['aligned'])
        b = int(c['rois'][r, 0])
        row = int(np.nonzero(np.abs(one[b]).sum((1, 2)))[0][1])                        # the second row of the roi's footprint
        wrong = g.copy()
        wrong[b, row] -= one[b, row]
        assert ref.check(g + 0.5 * bound, g, bound) < 0.51
        with pytest.raises(AssertionError):
            ref.check(wrong, g, bound, 'row dropped')
        assert (bound[UNNAMED] == (0 if into is None else ref.SLACK * (ref.U * np.abs(into[UNNAMED].astype(np.float64))))).all()


def test_check_bwd_accepts_the_footprint_and_nothing_outside_it():
    c = rc.grid_case(rc.NONFINITE_BWD[0])
    d, which = rc.plant_nonfinite_dout(c)
    shape = (c['B'], c['H'], c['W'], c['C'])
    g, bound = ref.roi_align_bwd(d, shape, c['rois'], c['scale'], c['S'], c['aligned'], with_bound=True)
    may = ref.footprint_mask(shape, c['rois'], c['scale'], c['P'], c['S'], c['aligned'], which)
    assert ref.check_bwd(g, g, bound, may) == 0.0
    assert ref.check_bwd(np.where(may, np.nan, g), g, bound, may) == 0.0                # the tiled path's pattern
    with pytest.raises(AssertionError):
        ref.check_bwd(np.nan_to_num(g, nan=0.0), g, bound, may)                          # the NaN lost
    wrong = g.copy()
    wrong[UNNAMED, 0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        ref.check_bwd(wrong, g, bound, may)
    wrong = g.copy()
    k = tuple(np.argwhere(may & np.isfinite(g))[0])
    wrong[k] += 3 * bound[k] + 1e-30
    with pytest.raises(AssertionError):
        ref.check_bwd(wrong, g, bound, may)
