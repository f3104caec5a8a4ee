"""CPU checks of the fused-loss restatement (tests/loss_ref.py) and of the cases the direct GPU tests run (tests/loss_cases.py).

1. The restatement is pinned to the repository's tensor-expression path, Detect.matcher + DetLoss on the CPU in fp32, for every case:
   candidate lists and target boxes equal row for row, the loss within rtol 2e-4, the logits gradient within test_gpu_loss_forms.elementwise
   (rtol 1e-4, 2e-5 rms per level) wherever the fp32 autograd is finite.  Every geometry is expressed by a real Detect whose anchor buffers
   are set to the case's grid-unit anchors.  Two regions are not compared, both documented holes of the reference that loss_ref defines as
   csrc/loss.hip does: elements where the fp32 autograd is not finite (saturated sigmoids), and the box and objectness logits of a
   (cell, anchor) with a candidate whose predicted w or h lies below the 1e-12 floor (4 s^2 anchor < 1e-12 from a logit of about -14.5 on:
   there the reference is still finite and uses the unfloored value, so the floor is a deviation of the kernel's definition from the
   reference, small in value and confined to those logits).  Those regions are pinned by loss_ref(float32) against loss_ref(float64).
2. Each case contains what it is for: counts asserted below, so that an edited case that loses its feature fails here.
"""
import functools

import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_ref
from hd_yolo_amd import synth  # noqa: F401  (makes `metayolo` importable)


def level_view(t, na, no):
    B, ny, nx, _ = t.shape
    return t[..., :na * no].reshape(B, ny, nx, na, no).permute(0, 3, 1, 2, 4)


@functools.lru_cache(maxsize=None)
def head_of(gname, form):
    from metayolo.models.yolo_head import Detect
    geom = lc.GEOMS[gname]
    hyp, gr, sort = lc.form_of(form, geom['nc'])
    nl, na, nc = geom['nl'], geom['na'], geom['nc']
    head = Detect([4] * nl, [[8, 8] * na] * nl, [8] * nl, nc, masks={i: -1 for i in range(nc + 1)}, loss_hyp=hyp, default_input_size=None)
    for buf, anc in zip(head.anchors, geom['anchors']):
        buf.anchor = torch.from_numpy(np.array(anc))                  # grid units, the exact float32 values of the case
    assert head.na == na and head.nl == nl and head.nc_masks == 0
    head.det_loss.gr, head.det_loss.sort_obj_iou = gr, sort
    assert head.det_loss.balance[:nl] == geom['balance']
    return head


def tensor_path(name):
    """Detect.matcher + DetLoss in fp32 on the CPU: (loss, items, per-level gradient (B, na, ny, nx, no), matcher output)"""
    c = lc.inputs_of(name)
    geom = c['geom']
    head = head_of(geom['name'], name.split('-')[3])
    dets = [level_view(x, geom['na'], geom['no']).clone().requires_grad_(True) for x in c['logits']]
    gts = torch.from_numpy(c['gts'])
    labels = torch.cat([torch.zeros((len(gts), 1)), torch.from_numpy(c['tcls'])], 1)
    tbox, tids, indices, anch = head.matcher(dets, gts)
    loss, items = head.det_loss(dets, [labels[i] for i in tids], tbox, indices, anch)
    grads = torch.autograd.grad(loss.sum(), dets, allow_unused=True)
    return loss.detach(), items, [torch.zeros_like(d) if g is None else g for g, d in zip(grads, dets)], (tbox, tids, indices)


@pytest.mark.parametrize('name', lc.CASES)
def test_restatement_equals_the_tensor_expression_path(name):
    c = lc.inputs_of(name)
    geom = c['geom']
    na, no = geom['na'], geom['no']
    ref = lc.ref_of(name)
    loss, items, grads, (tbox, tids, indices) = tensor_path(name)
    compared = 0
    clean = True
    for l, m in enumerate(ref['cands']):
        b, a, gj, gi = indices[l]
        for got, want in ((b, m['b']), (a, m['a']), (gj, m['gj']), (gi, m['gi']), (tids[l], m['g'])):
            assert np.array_equal(got.numpy(), want), (name, l)
        if len(m['g']):
            assert np.array_equal(tbox[l].numpy(), m['tbox']), (name, l)                  # float32, bit for bit
        got = grads[l].double()
        want = level_view(ref['grads'][l], na, no)
        use = torch.isfinite(got)
        fl = m['floored']
        if fl.any():
            use[torch.from_numpy(m['b'][fl]), torch.from_numpy(m['a'][fl]), torch.from_numpy(m['gj'][fl]), torch.from_numpy(m['gi'][fl]), :5] = False
        clean = clean and bool(torch.isfinite(got).all()) and not fl.any()
        rms = want.pow(2).mean().sqrt().item() + 1e-30
        err = ((got - want).abs() - 1e-4 * want.abs())[use]
        compared += int(use.sum())
        if err.numel():
            assert err.max().item() / rms <= 2e-5, (name, l, err.max().item() / rms)
        assert (ref['grads'][l][..., na * no:] == 0).all()
    kind = name.split('-')[2]
    assert clean or kind in ('sat',), name                  # only saturated logits may leave the reference's finite, unfloored range
    assert compared > 0
    if clean:
        np.testing.assert_allclose(ref['loss'], loss.item(), rtol=2e-4)
        for k, key in (('box', 'lbox'), ('obj', 'lobj'), ('cls', 'lcls')):
            np.testing.assert_allclose(ref[key], items[k].item(), rtol=2e-4, atol=1e-12)


@pytest.mark.parametrize('name', lc.HARD)
def test_float64_restatement_is_finite_where_float32_arithmetic_is_stressed(name):
    """saturated and planted logits: every value of the float64 run is finite, and so is the float32 run of the same code (the yardstick)"""
    for dtype in (torch.float64, torch.float32):
        r = lc.ref_of(name, dtype)
        assert np.isfinite([r['loss'], r['lbox'], r['lobj'], r['lcls']]).all(), (name, dtype)
        assert all(torch.isfinite(g).all() for g in r['grads']), (name, dtype)
    np.testing.assert_allclose(lc.ref_of(name, torch.float32)['loss'], lc.ref_of(name)['loss'], rtol=2e-4)


# ------------------------------------------------------------------------------------------ what each case contains
def lists_of(m, na, ny, nx):
    """records per (image, anchor, cell) of one level"""
    lin = ((m['b'] * na + m['a']) * ny + m['gj']) * nx + m['gi']
    return np.unique(lin, return_counts=True)[1] if len(lin) else np.zeros(0, np.int64)


@pytest.mark.parametrize('gname', ['G1', 'G2', 'G3', 'G4', 'G5a', 'G5b'])
def test_lattice_and_pile_contain_their_features(gname):
    geom = lc.GEOMS[gname]
    ref = lc.ref_of(f'{gname}-latpile-u12-bce')
    gts, tcls, tags = lc.targets_of(gname, 'latpile')
    m0 = ref['cands'][0]
    ny, nx = geom['grids'][0]
    assert set(np.concatenate([m['j'] for m in ref['cands']]).tolist()) == {0, 1, 2, 3, 4}        # every offset variant
    assert any(m['clamped'].any() for m in ref['cands'])                                          # cx = 1 or cy = 1: a clamped cell
    assert all(len(m['g']) > 0 for m in ref['cands'])                                             # every level has matches
    counts = np.concatenate([lists_of(m, geom['na'], *g) for m, g in zip(ref['cands'], geom['grids'])])
    assert (counts >= 3).any()
    if gname not in ('G5a', 'G5b'):                       # one 4 x 4 level: every list there is long
        assert (counts == 2).any() and (counts == 1).any()
    if gname == 'G1':
        # on the 8-grid every lattice centre is on a cell or half-cell boundary, and borders 0 and 1 are present
        lat = gts[:tags['pile']]
        assert (np.fmod(lat[:, 1:3] * np.float32(8), np.float32(0.5)) == 0).all()
        assert lat[:, 1].min() == 0 and lat[:, 1].max() == 1 and lat[:, 2].min() == 0 and lat[:, 2].max() == 1
    if geom['nl'] == 5:
        m = ref['cands'][4]                                                                       # the 1 x 1 level: only the centre cell
        assert len(m['g']) and set(m['j'].tolist()) == {0} and not m['gi'].any() and not m['gj'].any()
    # class rows: one-hot, multi-hot and all-zero rows among the matched targets; some image without ... see the edges set
    matched = np.unique(np.concatenate([m['g'] for m in ref['cands']]))
    hot = tcls[matched].sum(1)
    assert (hot == 0).any() and (hot == 1).any() and (geom['nc'] == 1 or (hot == 2).any())
    # the pile: 40 records in its centre cell for anchor 0 of level 0, in enumeration order after the lattice's
    p0 = tags['pile']
    cell = (m0['j'] == 0) & (m0['a'] == 0) & (m0['b'] == 0) & (m0['gj'] == 2) & (m0['gi'] == 3)
    in_pile = cell & (m0['g'] >= p0)
    assert in_pile.sum() == lc.PILE_N and np.array_equal(m0['g'][in_pile], np.arange(p0, p0 + lc.PILE_N))
    iou = m0['iou'][in_pile]
    assert (np.abs(np.diff(iou)) >= 0.05).all(), np.abs(np.diff(iou)).min()                      # a wrong winner moves the target by >= 0.05
    same = list(lc.PILE_SAME)
    assert (gts[p0 + np.array(same)] == gts[p0]).all() and (iou[same] == iou[0]).all() and iou[0] > 0.999
    every = m0['iou'][(m0['a'] == 0) & (m0['b'] == 0) & (m0['gj'] == 2) & (m0['gi'] == 3)]     # the whole list of that (cell, anchor)
    assert len(every) >= lc.PILE_N and every.max() == iou[0] and (every == every.max()).sum() >= 3   # sort_obj_iou: the maximum is a tie
    order_last = np.nonzero((m0['a'] == 0) & (m0['b'] == 0) & (m0['gj'] == 2) & (m0['gi'] == 3))[0][-1]
    assert every.max() - m0['iou'][order_last] >= 0.05                                            # last candidate and best IoU disagree


@pytest.mark.parametrize('gname', ['G1', 'G2', 'G3', 'G4', 'G5a', 'G5b'])
def test_edge_targets_contain_their_features(gname):
    geom = lc.GEOMS[gname]
    gts, _, tags = lc.targets_of(gname, 'edges')
    ny, nx = geom['grids'][0]
    m = loss_ref.match_level(gts, geom['anchors'][0], ny, nx, lc.ANCHOR_T)
    anchor0 = {int(g) for g, a in zip(m['g'], m['a']) if a == 0}
    assert len(tags['ratio']) >= 2                           # both lower edges; an upper edge too where 4 * anchor fits the image
    for at, inside in tags['ratio']:
        assert m['ratio'][0, at] == np.float32(lc.ANCHOR_T) and at not in anchor0                 # rejected at ratio == anchor_t exactly
        assert m['ratio'][0, inside] < np.float32(lc.ANCHOR_T) and inside in anchor0              # accepted one step inside
        side = 3 if gts[at, 3] != gts[inside, 3] else 4
        assert abs(int(gts[at, side].view(np.int32)) - int(gts[inside, side].view(np.int32))) <= 2   # ... which is an ulp or two of the side
    for g in tags['degenerate']:
        assert not (m['g'] == g).any() and (gts[g, 3] == 0 or gts[g, 4] == 0)
        assert all(not (loss_ref.match_level(gts, geom['anchors'][l], *geom['grids'][l], lc.ANCHOR_T)['g'] == g).any() for l in range(geom['nl']))
    # one ulp below a half-cell boundary the left / upper neighbour is taken (variant 1 / 2), one ulp above it is not (variants 3 / 4 see
    # nx - gx, whose float32 rounding absorbs the ulp: decided by the arithmetic, not asserted here); one ulp around a cell boundary the
    # centre cell itself changes
    for tag, jlow, col in (('ulp_x', 1, 'gi'), ('ulp_y', 2, 'gj')):
        has = {(int(g), int(j)) for g, j in zip(m['g'], m['j'])}
        n_half = n_cell = 0
        cells = {}
        for g, side, half in tags[tag]:
            v = float(gts[g, 1 if tag == 'ulp_x' else 2] * np.float32(nx if tag == 'ulp_x' else ny))       # the float32 product
            if not any(gg == g for gg, _ in has):
                continue
            if half and 1.5 < v < (nx if tag == 'ulp_x' else ny) - 1.5 and v % 1 != 0.5:      # (on a grid of 10 the product may absorb the ulp)
                assert ((g, jlow) in has) == (side == 'below'), (g, side)
                n_half += 1
            if not half:
                cells[(round(v), side)] = int(m[col][(m['g'] == g) & (m['j'] == 0)][0])
        for (k, side), cell in cells.items():
            if side == 'above' and (k, 'below') in cells:
                assert cell == cells[(k, 'below')] + 1
                n_cell += 1
        assert n_half >= 2 and n_cell >= 2, (tag, n_half, n_cell)
    if geom['B'] > 1:
        assert (gts[:, 0] == 0).all()                                                             # the other images have no target


@pytest.mark.parametrize('gname', ['G1', 'G2', 'G3', 'G4', 'G5a', 'G5b'])
def test_planted_and_saturated_logits_contain_their_features(gname):
    ref = lc.ref_of(f'{gname}-latpile-planted-bce')
    inter = np.concatenate([m['inter'] for m in ref['cands']])
    plain = np.concatenate([m['iou_plain'] for m in ref['cands']])
    v = np.concatenate([m['v'] for m in ref['cands']])
    assert (inter == 0).sum() >= 3                           # the clamp0 branch
    assert (plain > 0.999).sum() >= 3 and (v[plain > 0.999] < 1e-9).all()      # prediction == target: IoU ~ 1, v = 0
    assert ((v < 1e-12) & (plain > 0.27) & (plain < 0.29)).sum() >= 3          # same aspect ratio at 0.53 of the size: IoU 0.28, v = 0
    sat = lc.logits_of(gname, 'latpile', 'sat')
    vals = torch.cat([x.flatten() for x in sat])
    for s in lc.SAT_VALUES.tolist():
        assert (vals == s).any()
    assert any(m['floored'].any() for m in lc.ref_of(f'{gname}-latpile-sat-bce')['cands'])       # the 1e-12 floor acts


def test_channel_groups_straddle_anchors_where_the_pitch_is_no_multiple_of_the_outputs():
    """dense_kernel handles 4 channels per lane.  With no % 4 != 0 a group can hold the tail of one anchor and the head of the next: its
    second half then holds box channels of anchor a0 + 1, and the objectness channel of a straddling group is always in its FIRST half
    (it is output 4 of its anchor and the group is 4 wide: 4 + no - o0 < 4 has no solution), so the case the kernel's `a4 = a0 + 1`
    arm would serve cannot occur with valid sizes.  Asserted: straddling groups exist in G2, G3 and G4 (in G2 and G3, no <= 7, also ones whose first half holds
    the objectness channel), not in G1; padding-only groups exist where ldg > na * no."""
    def groups(geom):
        na, no = geom['na'], geom['no']
        out = []
        for c0 in range(0, geom['ldg'], 4):
            ch = [(c // no, c % no) for c in range(c0, c0 + 4) if c < na * no]
            out.append(ch)
        return out
    for gname, want in (('G1', False), ('G2', True), ('G3', True), ('G4', True), ('G5a', True), ('G5b', True)):
        gs = groups(lc.GEOMS[gname])
        two = [g for g in gs if len({a for a, _ in g}) == 2]
        assert bool(two) == want, gname
        for g in two:
            a0 = g[0][0]
            assert all(o != 4 for a, o in g if a != a0)                    # never an objectness channel in the second half
        if want and lc.GEOMS[gname]['no'] <= 7:                            # the tail of an anchor reaches back to its output 4
            assert any(any(a == g[0][0] and o == 4 for a, o in g) for g in two)
        if want:
            assert any(any(a != g[0][0] and o < 4 for a, o in g) for g in two)
    assert any(not g for g in groups(lc.GEOMS['G1'])) and any(not g for g in groups(lc.GEOMS['G4']))
    assert any(0 < len(g) < 4 for g in groups(lc.GEOMS['G2']))             # a group that is part channels, part padding


def test_g6_makes_a_second_trip_and_long_lists():
    geom = lc.GEOMS['G6']
    gts, _, _ = lc.targets_of('G6', 'g6')
    assert len(gts) == lc.G6_NT and 5 * geom['na'] * len(gts) > 1024 * 1024        # more candidates than one grid pass of match_kernel
    m = lc.ref_of('G6-g6-u1-bce')['cands'][0]
    counts = lists_of(m, 1, 32, 32)
    assert len(counts) == 4 * 32 * 32 and counts.max() >= 100 and np.median(counts) >= 50
    assert set(m['j'].tolist()) == {0, 1, 2, 3, 4} and m['clamped'].any()
    on = np.fmod(gts[:, 1] * np.float32(32), np.float32(0.5)) == 0
    assert 0.15 < on.mean() < 0.4                                                  # exact boundary centres and jittered ones


def test_mask_selection_cases_are_well_posed():
    """the targets of the mask-selection test: every kept target's best level is ahead of its other levels by far more than the float32
    noise of the decode, or all its IoUs are exactly zero (then the first level wins on both sides)"""
    geom = lc.GEOMS['G1']
    for tset in ('latpile', 'edges'):
        gts, _, _ = lc.targets_of('G1', tset)
        r = loss_ref.mask_select(lc.logits_of('G1', tset, 'u1'), gts, geom['anchors'], geom['nc'], geom['strides'], lc.ANCHOR_T, 0.0)
        keep = r['keep']
        any_level = np.unique(np.concatenate([loss_ref.match_level(gts, geom['anchors'][l], *geom['grids'][l], lc.ANCHOR_T)['g']
                                              for l in range(geom['nl'])]))
        assert np.array_equal(keep, any_level) and len(keep) > 0 and (len(keep) < len(gts) or tset == 'latpile')   # edges: degenerate rows drop out
        assert sum(r['counts']) == len(keep) and sum(c > 0 for c in r['counts']) >= 2
        gap = r['gap'][keep]
        assert ((gap > 1e-4) | ((gap == 0) & (r['best'][keep] == 0))).all(), gap.min()


def test_stale_workspace_sequence_shrinks():
    big, small, none = (len(lc.targets_of('G1', t)[0]) for t in ('latpile', 'small', 'empty'))
    assert big > 64 > small > none == 0
    assert sum(len(m['g']) for m in lc.ref_of('G1-small-u12-bce')['cands']) > 0
