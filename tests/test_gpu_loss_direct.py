"""csrc/loss.hip driven directly (ops.DetLossCall, no model) on an MI355X against the float64 restatement tests/loss_ref.py, on the cases of
tests/loss_cases.py (tests/test_loss_ref_host.py proves on the CPU what each contains: centres on cell and half-cell boundaries and one ulp
off them, clamped cells, sides at the anchor-ratio threshold, degenerate rows, a pile of 40 targets in one cell, saturated and planted
logits, groups of 4 channels that straddle anchors, MAXL levels / MAXA anchors / MAXC classes, a 1 x 1 level, 212 000 targets).

Criteria: out[0..3] within rtol 2e-4; the fp32 logits gradient within elementwise() <= 2e-5 per level (rtol 1e-4 and 2e-5 of the level's
rms: the project's figures, tests/test_gpu_loss_forms.py), every element finite, padding channels exactly zero, the 7.0 prefill gone
everywhere; the bf16 gradient bit-equal to the fp32 one rounded once (.to(torch.bfloat16), round to nearest even).

Yardstick rule for saturated and planted logits (loss_cases.HARD): where a level misses 2e-5, its bound is four times the error of
loss_ref(float32) against loss_ref(float64) on the same case, i.e. four times what a plain float32 evaluation of the same formulas loses;
the factor covers the kernel's dual-number operation order, differently associated sums and fp64 means.  The bound never comes from the
kernel's output.  Measured on an MI355X, worst level of each case, in elementwise() units (the figure that must stay <= 2e-5;
0 = inside rtol 1e-4 everywhere).  Every case meets the plain criterion by a factor of 40 or more, so the yardstick arm has not been needed:

    case                        kernel (level)    float32 restatement (level)
    G1-latpile-sat-bce          2.24e-08 (2)      8.26e-09 (2)
    G1-latpile-planted-bce      4.39e-07 (0)      3.33e-07 (0)
    G1-edges-sat-bce            1.43e-08 (0)      1.15e-08 (1)
    G1-edges-planted-bce        1.65e-09 (1)      9.48e-10 (0)
    G2-latpile-sat-bce          5.57e-09 (2)      2.85e-09 (0)
    G2-latpile-planted-bce      5.30e-08 (0)      1.63e-08 (0)
    G2-edges-sat-bce            3.74e-09 (1)      3.74e-09 (1)
    G2-edges-planted-bce        1.49e-09 (1)      8.14e-10 (0)
    G3-latpile-sat-bce          3.60e-08 (1)      8.38e-09 (0)
    G3-latpile-planted-bce      1.34e-07 (0)      1.75e-07 (0)
    G3-edges-sat-bce            7.69e-08 (0)      2.24e-08 (1)
    G3-edges-planted-bce        1.67e-09 (0)      1.31e-09 (0)
    G4-latpile-sat-bce          5.63e-08 (0)      1.02e-07 (0)
    G4-latpile-planted-bce      1.86e-07 (1)      2.60e-07 (1)
    G4-edges-sat-bce            8.36e-08 (2)      3.03e-08 (2)
    G4-edges-planted-bce        5.03e-07 (1)      5.03e-07 (1)
    G5a-latpile-sat-bce         4.02e-09 (0)      2.14e-09 (0)
    G5a-latpile-planted-bce     0.00e+00 (0)      0.00e+00 (0)
    G5a-edges-sat-bce           4.20e-09 (0)      2.18e-09 (0)
    G5a-edges-planted-bce       2.09e-09 (0)      5.53e-10 (0)
    G5b-latpile-sat-bce         2.29e-09 (0)      2.29e-09 (0)
    G5b-latpile-planted-bce     0.00e+00 (0)      0.00e+00 (0)
    G5b-edges-sat-bce           3.00e-09 (0)      3.00e-09 (0)
    G5b-edges-planted-bce       2.29e-09 (0)      7.79e-10 (0)
    G1-latpile-sat-focal05      3.09e-08 (2)      1.14e-08 (2)
    G3-latpile-sat-focal05      1.31e-08 (0)      1.14e-08 (0)

    For comparison, the unsaturated cases: worst 5.9e-7 (G6, lists of > 100 records), typically 1e-9 .. 4e-7.

Repeat determinism and stale workspaces: the record region of the workspace is never zeroed, so a call after a larger one sees the larger
one's records behind its own; results must be bit-equal to a fresh DetLossCall.  No index-carrying buffer is filled with a pattern here
(the safety rule of tests/test_gpu_scratch.py): the stale records come from a valid call and hold in-range links.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import loss_cases as lc  # noqa: E402
import loss_ref  # noqa: E402
from hd_yolo_amd import ops  # noqa: E402

DEV = torch.device('cuda', 0)
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def bits(t):
    return t.contiguous().view(INT_VIEW[t.dtype])


class Direct:
    """one DetLossCall on a case's logits, with fresh 7.0-filled gradient buffers"""

    def __init__(self, name, dtype=torch.float32):
        from metayolo.models.loss import DetLoss
        c = lc.inputs_of(name)
        geom = c['geom']
        self.case, self.geom = c, geom
        self.logits = [x.to(DEV).contiguous() for x in c['logits']]
        self.gdets = [torch.full(tuple(x.shape[:3]) + (geom['ldg'],), 7.0, dtype=dtype, device=DEV) for x in self.logits]
        self.out = torch.full((4,), 7.0, dtype=torch.float32, device=DEV)
        dl = DetLoss(geom['nc'], geom['nl'], c['hyp'])
        dl.gr, dl.sort_obj_iou = c['gr'], c['sort']
        assert list(dl.balance)[:geom['nl']] == geom['balance']
        cw, pw = lc.class_weights(c['hyp'], geom['nc'])
        self.call = ops.DetLossCall(self.logits, self.gdets, geom['na'], geom['nc'], geom['anchors'].flatten().tolist(), dl.balance, cw, pw,
                                    c['hyp']['obj_pw'], dl, self.out, DEV)

    def run(self, gts=None, tcls=None):
        gts = self.case['gts'] if gts is None else gts
        tcls = self.case['tcls'] if tcls is None else tcls
        self.targets = (torch.from_numpy(gts).to(DEV).contiguous(), torch.from_numpy(tcls).to(DEV).contiguous())
        self.call(*self.targets)
        torch.cuda.synchronize()
        return self.out.clone(), [g.clone() for g in self.gdets]


def check_against_restatement(name, out, gdets):
    geom = lc.inputs_of(name)['geom']
    used = geom['na'] * geom['no']
    ref = lc.ref_of(name)
    hard = name in lc.HARD
    ref32 = lc.ref_of(name, torch.float32) if hard else None
    want = np.array([ref[k] for k in ('loss', 'lbox', 'lobj', 'lcls')])
    print(name, 'out', out.tolist(), 'ref', want.tolist())
    figures = []
    for l, (g, r) in enumerate(zip(gdets, ref['grads'])):
        e = lc.elementwise(g[..., :used], r[..., :used])
        y = lc.elementwise(ref32['grads'][l][..., :used], r[..., :used]) if hard else float('nan')
        figures.append((l, e, y))
        print(f'{name} level {l}: kernel {e:.3e} yardstick {y:.3e}')
    assert torch.isfinite(out).all(), out
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=2e-4, atol=1e-12)
    for (l, e, y), g in zip(figures, gdets):
        assert torch.isfinite(g).all(), (name, l)
        assert (g != 7.0).all(), (name, l)                                       # every element overwritten
        assert (g[..., used:] == 0).all(), (name, l)                             # padding channels exactly zero
        assert e <= 2e-5 or (hard and e <= 4 * y), (name, l, e, y)


@pytest.mark.parametrize('name', lc.CASES)
def test_fused_loss_matches_the_float64_restatement(name):
    """fp32 gradient buffers against loss_ref(float64); bf16 buffers bit-equal to those rounded once"""
    out, gdets = Direct(name).run()
    check_against_restatement(name, out, gdets)
    out16, g16 = Direct(name, torch.bfloat16).run()
    np.testing.assert_allclose(out16.cpu().numpy(), out.cpu().numpy(), rtol=1e-6)          # fp64 atomics in any order, rounded to fp32
    for l, (a, b) in enumerate(zip(g16, gdets)):
        assert torch.equal(bits(a), bits(b.to(torch.bfloat16))), (name, l)


@pytest.mark.parametrize('name', ['G6-g6-u1-bce', 'G1-latpile-u12-bce', 'G3-latpile-u12-sort_gr05'])
def test_two_calls_give_the_same_bits(name):
    """lists of 40 to a few hundred records, summed in candidate order whatever order they arrived in"""
    d = Direct(name)
    out0, g0 = d.run()
    for g in d.gdets:
        g.fill_(7.0)
    out1, g1 = d.run()
    for l, (a, b) in enumerate(zip(g0, g1)):
        assert torch.equal(bits(a), bits(b)), (name, l)
    np.testing.assert_allclose(out1.cpu().numpy(), out0.cpu().numpy(), rtol=1e-6)
    _, g = Direct(name).run()
    for l, (a, b) in enumerate(zip(g0, g)):
        assert torch.equal(bits(a), bits(b)), (name, l)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_stale_workspace_is_never_read(dtype):
    """one DetLossCall: the pile (many records), then 7 targets, then none; each bit-equal to the same call on a fresh DetLossCall"""
    big, small, none = 'G1-latpile-u12-bce', 'G1-small-u12-bce', 'G1-empty-u1-bce'
    d = Direct(big, dtype)
    d.run()
    ws_after_big = d.call.ws
    for name in (small, none, small):
        c = lc.inputs_of(name)
        for g in d.gdets:
            g.fill_(7.0)
        out, gdets = d.run(c['gts'], c['tcls'])
        assert d.call.ws is ws_after_big                                         # the same, unzeroed, workspace
        fresh = Direct(big, dtype)                                               # the same logits, a workspace of its own
        want_out, want = fresh.run(c['gts'], c['tcls'])
        assert torch.equal(out, want_out), (name, out, want_out)
        for l, (a, b) in enumerate(zip(gdets, want)):
            assert torch.equal(bits(a), bits(b)), (name, l)
    # and the results are right, not only equal: the 7-target call against the restatement on the big case's logits
    c = lc.inputs_of(small)
    geom, hyp = c['geom'], c['hyp']
    cw, pw = lc.class_weights(hyp, geom['nc'])
    ref = loss_ref.det_loss(lc.inputs_of(big)['logits'], c['gts'], c['tcls'], geom['anchors'], geom['nc'], geom['balance'], cw, pw, hyp['obj_pw'],
                            hyp['anchor_t'], hyp['label_smoothing'], hyp['box'], hyp['obj'], hyp['cls'])
    np.testing.assert_allclose(out.cpu().numpy(), [ref[k] for k in ('loss', 'lbox', 'lobj', 'lcls')], rtol=2e-4)
    if dtype == torch.float32:
        used = geom['na'] * geom['no']
        for l, (g, r) in enumerate(zip(gdets, ref['grads'])):
            assert lc.elementwise(g[..., :used], r[..., :used]) <= 2e-5, l


@pytest.mark.parametrize('tset', ['latpile', 'edges'])
def test_mask_selection_runs_the_same_matcher(tset):
    """hdy_mask_select's copy of the matcher, min_iou 0: the kept targets are exactly those with a candidate on some level, in target order
    (the order of the tensor-expression selection in tests/test_gpu_mask.py), and the per-level counts are the restatement's"""
    name = f'G1-{tset}-u1-bce'
    d = Direct(name)
    c, geom = d.case, d.geom
    gts = torch.from_numpy(c['gts']).to(DEV).contiguous()
    apx = [float(v) * s for anc, s in zip(geom['anchors'], geom['strides']) for v in anc.flatten()]
    counts, keep_t, rois, order = d.call.mask_select(gts, apx, geom['strides'], min_iou=0.0)
    torch.cuda.synchronize()
    counts = counts.tolist()
    ref = loss_ref.mask_select(c['logits'], c['gts'], geom['anchors'], geom['nc'], geom['strides'], lc.ANCHOR_T, 0.0)
    assert counts[0] == len(ref['keep'])
    assert np.array_equal(keep_t[:counts[0]].cpu().numpy(), ref['keep'])
    assert counts[1:] == ref['counts'], (counts, ref['counts'])
    pos = torch.sort(order[:counts[0]].cpu()).values
    assert torch.equal(pos, torch.arange(counts[0]))                                      # a permutation of the kept rows
