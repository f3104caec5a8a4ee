"""The other DetLoss forms on a real MI355X: focal loss (fl_gamma > 0), the objectness target options gr < 1 and sort_obj_iou, and per-class
cls_pw, through csrc/loss.hip (hdy_det_loss_ex) and through the tensor-expression DetLoss, against the reference's goldens
(tests/golden/make_golden_loss_forms.py) with the criteria of tests/test_gpu_model.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hd_yolo_amd import _lib, ops, synth  # noqa: E402

DEV = 'cuda:0'
TRAIN = ['focal_n_64_ragged', 'focal_s_128', 'iou_target_n_256', 'clspw_n_64']


def form_of(g):
    """the loss options a fixture was made with"""
    def opt(a):
        a = np.asarray(a, dtype=np.float64)
        return float(a) if a.ndim == 0 else [float(v) for v in a]
    return {'fl_gamma': opt(g['hyp_fl_gamma']), 'label_smoothing': opt(g['hyp_label_smoothing']), 'cls_pw': opt(g['hyp_cls_pw']),
            'obj_pw': opt(g['hyp_obj_pw']), 'cls_cw': opt(g['hyp_cls_cw']), 'gr': float(g['gr']), 'sort_obj_iou': bool(int(g['sort_obj_iou']))}


def build(variant, nc, form):
    from metayolo.models.yolo import Model
    hyp = synth.make_hyp()
    hyp['det'].update({k: v for k, v in form.items() if k not in ('gr', 'sort_obj_iou')})
    model = Model(synth.make_cfg(variant, nc), hyp)
    sd = synth.synth_state_dict(synth.shapes_of(model), seed=0)
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys
    dl = model.headers['det'].det_loss
    dl.gr, dl.sort_obj_iou = form.get('gr', 1.0), form.get('sort_obj_iou', False)
    return model.to(DEV)


def targets_of(g):
    batch, size, nc, nmin, nmax = (int(v) for v in g['meta'][:5])
    targets = synth.synth_targets(batch, size, nc, nmin=nmin, nmax=nmax, seed=5)
    if 'empty_first' in g.files and int(g['empty_first']):
        a = targets[0]['anns']['det'][0]
        a['boxes'], a['labels'] = a['boxes'][:0], a['labels'][:0]
    return targets


def variant_of(name):
    return {'focal_n_64_ragged': 'n', 'focal_s_128': 's', 'iou_target_n_256': 'n', 'clspw_n_64': 'n', 'focal_n_128': 'n'}[name]


def relmax(got, ref):
    got, ref = torch.as_tensor(got).float().cpu(), torch.as_tensor(ref).float().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-12)).item()


def elementwise(got, ref, rtol=1e-4, arms=2e-5):
    """tests/test_gpu_model.py's criterion: the worst |error| - rtol * |ref| in units of rms(ref)"""
    got, ref = torch.as_tensor(got).float().cpu(), torch.as_tensor(ref).float().cpu()
    rms = ref.pow(2).mean().sqrt().item() + 1e-30
    return ((got - ref).abs() - rtol * ref.abs()).max().item() / rms


@pytest.fixture
def fused_calls(monkeypatch):
    """counts the hdy_det_loss_ex calls the model makes"""
    calls = []
    orig = ops.DetLossCall.__call__

    def counted(self, gts, tcls):
        calls.append(int(gts.shape[0]))
        return orig(self, gts, tcls)
    monkeypatch.setattr(ops.DetLossCall, '__call__', counted)
    return calls


@pytest.mark.parametrize('fused', ['1', '0'])
@pytest.mark.parametrize('name', TRAIN)
def test_train_step_forms_match_reference_golden_fp32(golden_dir, name, fused, monkeypatch, fused_calls):
    """test_train_step_matches_reference_golden_fp32's criteria for each loss form, on the fused loss ('1', which must have run) and on the
    tensor-expression DetLoss ('0')"""
    monkeypatch.setenv('HDY_FUSED_LOSS', fused)
    g = np.load(os.path.join(golden_dir, f'train_{name}.npz'))
    batch, size, nc, nmin, nmax = (int(v) for v in g['meta'])
    model = build(variant_of(name), nc, form_of(g)).train()
    x = synth.synth_images(batch, size, seed=11).to(DEV)
    losses, _ = model(x, targets_of(g), compute_masks=True)
    assert len(fused_calls) == (1 if fused == '1' else 0), fused_calls
    loss = losses['det']['det_loss'] + losses['det']['mask_loss']
    loss.backward()
    rtol = 2e-4
    np.testing.assert_allclose(losses['det']['det_loss'].detach().cpu().numpy(), g['loss'], rtol=rtol)
    for k in ('box', 'obj', 'cls'):
        np.testing.assert_allclose(losses['det']['loss_items'][k].cpu().numpy(), g[f'loss_{k}'], rtol=rtol)
    sd = model.state_dict()
    params = dict(model.named_parameters())
    for k in g.files:
        if k.startswith('stat:'):
            assert relmax(sd[k[5:]], g[k]) < 1e-4, k
        elif k.startswith('grad:'):
            assert relmax(params[k[5:]].grad, g[k]) < 1e-3, k
    bad = []
    for pname, (s, a, l2) in zip(g['gradsum_names'], g['gradsum']):
        gr = params[str(pname)].grad
        assert gr is not None, pname
        got = gr.double().pow(2).sum().sqrt().item()
        if abs(got - l2) > 2e-3 * l2 + 1e-9:
            bad.append((str(pname), got, l2))
    assert not bad, bad[:8]


def fused_step(model, x, targets):
    """forward + fused loss only: (plan, losses, per-level logits gradients as the plan holds them before its backward)"""
    head = model.headers['det']
    eng = model._eng()
    dtype = torch.float32
    plan, losses = head.fused_losses(eng, x, dtype, [t['anns']['det'][0] for t in targets])
    return plan, losses, [u.gdet.clone() for u in plan.det_units]


def level_view(t, na, no):
    """NHWC [B][ny][nx][ld] with channel a*no + o -> (B, na, ny, nx, no)"""
    B, ny, nx, _ = t.shape
    return t[..., :na * no].reshape(B, ny, nx, na, no).permute(0, 3, 1, 2, 4)


@pytest.mark.parametrize('name', TRAIN)
def test_fused_logits_gradient_matches_tensor_expression_autograd(golden_dir, name, fused_calls):
    """the gradient hdy_det_loss_ex writes into the plan's gradient buffers against autograd of the tensor-expression DetLoss on the same
    plan logits, level by level, fp32"""
    g = np.load(os.path.join(golden_dir, f'train_{name}.npz'))
    batch, size, nc = (int(v) for v in g['meta'][:3])
    model = build(variant_of(name), nc, form_of(g)).train()
    head = model.headers['det']
    x = synth.synth_images(batch, size, seed=11).to(DEV)
    targets = targets_of(g)
    plan, losses, gdets = fused_step(model, x, targets)
    assert len(fused_calls) == 1
    na, no = head.na, head.no
    dets = [level_view(u.logits, na, no).detach().clone().requires_grad_(True) for u in plan.det_units]
    ref = head.compute_losses(dets, [], None, [t['anns']['det'][0] for t in targets])
    grads = torch.autograd.grad(ref['det_loss'].sum(), dets)
    np.testing.assert_allclose(losses['det_loss'].detach().cpu().numpy(), ref['det_loss'].detach().cpu().numpy(), rtol=2e-4)
    for lvl, (gd, gref) in enumerate(zip(gdets, grads)):
        got = level_view(gd.float(), na, no)
        assert torch.isfinite(got).all(), lvl
        e = elementwise(got, gref)
        assert e <= 2e-5, (lvl, e)
        assert (gd[..., na * no:] == 0).all(), lvl                     # padding channels written as zero


def test_dense_cells_are_deterministic(golden_dir):
    """train_iou_target_n_256 (cells with 3 and more matches, sort_obj_iou, gr 0.5, focal): two runs give the same bits"""
    g = np.load(os.path.join(golden_dir, 'train_iou_target_n_256.npz'))
    batch, size, nc = (int(v) for v in g['meta'][:3])
    model = build('n', nc, form_of(g)).train()
    x = synth.synth_images(batch, size, seed=11).to(DEV)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        losses, _ = model(x, targets_of(g))
        plan = model._eng().plan_for(x, True, torch.float32)
        gdets = [u.gdet.clone() for u in plan.det_units]
        losses['det']['det_loss'].backward()
        runs.append((losses['det']['det_loss'].detach().clone(), gdets, {k: p.grad.clone() for k, p in model.named_parameters()}))
    (l0, g0, p0), (l1, g1, p1) = runs
    assert torch.equal(l0, l1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
    # the fixture has what it is meant to exercise: some (cell, anchor) with three matches or more on the largest level
    head = model.headers['det']
    gts, _ = head.flatten_targets([t['anns']['det'][0] for t in targets_of(g)], torch.device(DEV))
    dets = [level_view(u.logits, head.na, head.no) for u in plan.det_units]
    _, _, indices, _ = head.matcher(dets, gts)
    b, a, gj, gi = indices[0]
    lin = ((b * head.na + a) * dets[0].shape[2] + gj) * dets[0].shape[3] + gi
    assert torch.unique(lin, return_counts=True)[1].max().item() >= 3


def test_focal_train_step_bf16_is_close_to_fp32():
    """test_train_step_bf16_is_close_to_fp32 with fl_gamma 1.5"""
    nc = 8
    form = {'fl_gamma': 1.5}
    model = build('s', nc, form).train()
    x = synth.synth_images(4, 256, seed=11).to(DEV)
    t1 = synth.synth_targets(4, 256, nc, nmin=20, nmax=60, seed=5)
    t2 = synth.synth_targets(4, 256, nc, nmin=20, nmax=60, seed=5)
    ref_model = build('s', nc, form).train()
    l32, _ = ref_model(x, t1)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        l16, _ = model(x, t2)
    a, b = l32['det']['det_loss'].item(), l16['det']['det_loss'].item()
    assert abs(a - b) / a < 0.03, (a, b)
    l32['det']['det_loss'].backward()
    l16['det']['det_loss'].backward()
    p32, p16 = dict(ref_model.named_parameters()), dict(model.named_parameters())
    cos = {}
    for k in p32:
        u, v = p32[k].grad.flatten().double(), p16[k].grad.flatten().double()
        cos[k] = (torch.dot(u, v) / (u.norm() * v.norm() + 1e-30)).item()
    assert cos['headers.det.m.0.weight'] > 0.999 and cos['headers.det.m.2.bias'] > 0.999, cos
    vals = sorted(cos.values())
    assert vals[len(vals) // 2] > 0.85 and vals[0] > 0.6, (vals[0], vals[len(vals) // 2])


def test_focal_loss_trajectory_fp32_follows_the_reference(golden_dir, fused_calls):
    """trajectory_focal_n_128: fp32 SGD steps against the reference's losses; steps 0-3 within 2e-4 x 10^step, later steps within twice the
    reference's own spread (8 threads, weights perturbed by 1e-6), as test_loss_trajectory_fp32_follows_the_reference_and_bf16_stays_in_its_band"""
    from hd_yolo_amd.optim import SGD
    g = np.load(os.path.join(golden_dir, 'trajectory_focal_n_128.npz'))
    batch, size, nc, nmin, nmax, steps = (int(v) for v in g['meta'])
    ref = g['losses']
    model = build('n', nc, form_of(g)).train()
    x = synth.synth_images(batch, size, seed=11).to(DEV)
    targets = synth.synth_targets(batch, size, nc, nmin=nmin, nmax=nmax, seed=5)
    g_bn, g_w, g_b = [], [], []
    for m in model.modules():
        if hasattr(m, 'bias') and isinstance(m.bias, torch.nn.Parameter):
            g_b.append(m.bias)
        if isinstance(m, torch.nn.BatchNorm2d):
            g_bn.append(m.weight)
        elif hasattr(m, 'weight') and isinstance(m.weight, torch.nn.Parameter):
            g_w.append(m.weight)
    opt = SGD(g_bn, lr=float(g['lr']), momentum=float(g['momentum']), nesterov=True)
    opt.add_param_group({'params': g_w, 'weight_decay': float(g['weight_decay'])})
    opt.add_param_group({'params': g_b})
    losses = []
    for _ in range(steps):
        out, _ = model(x, targets)
        loss = out['det']['det_loss']
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss.detach()))
    assert len(fused_calls) == steps
    got = np.array(losses)
    rel = np.abs(got - ref) / ref
    own = max(float((np.abs(g['losses_8_threads'] - ref) / ref).max()), float((np.abs(g['losses_perturbed_1e6'] - ref) / ref).max()))
    print('focal trajectory: reference', ref[0], ref[-1], '| max rel', rel.max(), 'at step', int(rel.argmax()), '| band', 2 * own)
    assert (rel[:4] < 2e-4 * 10.0 ** np.arange(4)).all(), rel[:4]
    assert rel.max() < 2.0 * own, (rel.max(), own)
    assert got[-1] < 0.6 * got[0]


def loss_inputs(nc=2, size=256, B=2, nmin=60, nmax=200, seed=5, form=None, logits_fn=None):
    """A detection head's geometry and its det_loss (CPU model), random fp32 plan-layout logits and device targets"""
    from metayolo.models.yolo import Model
    hyp = synth.make_hyp()
    hyp['det'].update(form or {})
    head = Model(synth.make_cfg('n', nc), hyp).headers['det']
    na, no, nl = head.na, head.no, head.nl
    ld = (na * no + 3) // 4 * 4 + 4                       # a padded pitch, as the plans have
    gen = torch.Generator().manual_seed(seed)
    logits, anc = [], []
    for buf in head.anchors:
        n = int(size / float(buf.stride))
        t = torch.randn((B, n, n, ld), generator=gen) * 2.0
        if logits_fn is not None:
            t = logits_fn(t, na, no)
        logits.append(t.to(DEV).contiguous())
        anc += [float(v) for v in buf.anchor.flatten().tolist()]
    targets = synth.synth_targets(B, size, nc, nmin=nmin, nmax=nmax, seed=seed)
    gts, tcls = head.flatten_targets([t['anns']['det'][0] for t in targets], torch.device(DEV), fused=True)
    return head, logits, anc, ld, gts, tcls


def det_loss_call(head, logits, anc, ld, dtype):
    gdets = [torch.full((t.shape[0], t.shape[1], t.shape[2], ld), 7.0, dtype=dtype, device=DEV) for t in logits]
    out = torch.zeros(4, dtype=torch.float32, device=DEV)
    nc = head.nc
    call = ops.DetLossCall(logits, gdets, head.na, nc, anc, head.det_loss.balance, [1.0] * nc, [float(head.det_loss.hyp['cls_pw'])] * nc,
                           float(head.det_loss.hyp['obj_pw']), head.det_loss, out, torch.device(DEV))
    return call, gdets, out


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_old_entry_point_equals_the_bce_form_bitwise(dtype):
    """hdy_det_loss is hdy_det_loss_ex with the BCE form: the same out and logits gradient bits, fp32 and bf16 gradient buffers"""
    head, logits, anc, ld, gts, tcls = loss_inputs(nc=3)
    call, gdets, out = det_loss_call(head, logits, anc, ld, dtype)
    call(gts, tcls)
    torch.cuda.synchronize()
    ex = (out.clone(), [g.clone() for g in gdets])
    for g in gdets:
        g.fill_(3.0)
    out.zero_()
    h = head.det_loss.hyp
    nt = int(gts.shape[0])
    _lib.call('hdy_det_loss', call.lp, call.ldl, call.gp, call.ldg, call.dtype, call.ny, call.nx, call.nl, call.B, call.na, call.nc,
              call.anc, call.bal, gts.data_ptr(), tcls.data_ptr(), nt, call.cw, float(h['cls_pw']), float(h['obj_pw']), float(h['anchor_t']),
              float(h['label_smoothing']), float(h['box']), float(h['obj']), float(h['cls']), out.data_ptr(), call.ws.data_ptr(),
              call.ws.numel() * 4, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.isfinite(ex[0]).all() and ex[0][0] > 0
    assert torch.equal(out, ex[0]), (out, ex[0])
    for a, b in zip(gdets, ex[1]):
        assert torch.equal(a.view(torch.int16) if dtype == torch.bfloat16 else a.view(torch.int32),
                           b.view(torch.int16) if dtype == torch.bfloat16 else b.view(torch.int32))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_focal_gamma_below_one_with_saturated_objectness_is_finite(dtype):
    """gamma 0.5, objectness logits at +-30 (sigmoid saturates: q == 0 where the target is 0 and the logit -30): loss and gradients finite
    (the reference's autograd gives NaN there; csrc/loss.hip defines that term as its limit, 0)"""
    def saturate(t, na, no):
        for a in range(na):
            t[..., a * no + 4] = torch.where(torch.rand(t.shape[:3]) < 0.5, -30.0, 30.0)
            t[..., a * no + 5:a * no + no] = torch.where(torch.rand(t.shape[:3] + (no - 5,)) < 0.5, -25.0, 25.0)
        return t
    head, logits, anc, ld, gts, tcls = loss_inputs(form={'fl_gamma': 0.5, 'label_smoothing': 0.0}, logits_fn=saturate)
    head.det_loss.gr = 0.0                                 # matched cells get target 1: q == 0 at the logit +30 too
    call, gdets, out = det_loss_call(head, logits, anc, ld, dtype)
    call(gts, tcls)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), out
    for g in gdets:
        assert torch.isfinite(g.float()).all()
