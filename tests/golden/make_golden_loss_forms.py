#!/usr/bin/env python3
"""Golden vectors for the other DetLoss forms, from the REFERENCE's own Model / DetLoss on CPU (the shims, model construction and
fixture layout of make_golden.py):

    python tests/golden/make_golden_loss_forms.py

  train_focal_n_64_ragged.npz   fl_gamma 1.5, an empty first tile
  train_focal_s_128.npz         fl_gamma 2.0, label smoothing 0.1, per-class cls_pw and cls_cw, obj_pw 0.7
  train_iou_target_n_256.npz    fl_gamma 1.5, gr 0.5, sort_obj_iou (dense targets: cells with 3 and more matches)
  train_clspw_n_64.npz          BCE, per-class cls_pw
  trajectory_focal_n_128.npz    fl_gamma 1.5, 10 SGD steps (+ the reference's own spread: 8 threads, weights perturbed by 1e-6)
  keys_focal.npz                state-dict keys and shapes of focal models

Each fixture carries the loss options it was made with (`hyp_*` entries, `gr`, `sort_obj_iou`), so a test builds the same model from it.
Every forward runs on one host thread: with several matches in one cell the reference's parallel index_put keeps no fixed last write
(make_golden.gen_train).
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import GRAD_KEYS, STAT_KEYS, npf, ref_model  # noqa: E402

synth = mg.synth

FORMS = {
    'focal': {'fl_gamma': 1.5},
    'focal_s': {'fl_gamma': 2.0, 'label_smoothing': 0.1, 'cls_pw': [1.0, 2.0, 0.5], 'obj_pw': 0.7, 'cls_cw': [1.0, 0.5, 2.0]},
    'iou_target': {'fl_gamma': 1.5, 'gr': 0.5, 'sort_obj_iou': True},
    'clspw': {'cls_pw': [1.5, 0.5]},
}


def form_hyp(form):
    """synth.make_hyp() with the form's DetLoss options; gr / sort_obj_iou are attributes set after construction, not hyp entries"""
    hyp = synth.make_hyp()
    hyp['det'].update({k: v for k, v in form.items() if k not in ('gr', 'sort_obj_iou')})
    return hyp


def form_model(variant, nc, form):
    model = ref_model(variant, nc, form_hyp(form))
    dl = model.headers['det'].det_loss
    dl.gr = float(form.get('gr', 1.0))
    dl.sort_obj_iou = bool(form.get('sort_obj_iou', False))
    return model


def form_entries(form):
    h = form_hyp(form)['det']
    return {'hyp_fl_gamma': np.array(float(h['fl_gamma'])), 'hyp_label_smoothing': np.array(float(h['label_smoothing'])),
            'hyp_cls_pw': np.array(h['cls_pw'], dtype=np.float64), 'hyp_obj_pw': np.array(float(h['obj_pw'])),
            'hyp_cls_cw': np.array(h['cls_cw'], dtype=np.float64), 'gr': np.array(float(form.get('gr', 1.0))),
            'sort_obj_iou': np.array(int(bool(form.get('sort_obj_iou', False))))}


def gen_train_form(tag, variant, nc, batch, size, nmin, nmax, form, empty_first=False):
    """make_golden.gen_train's entries (loss, items, BN statistics, gradients, per-parameter gradient sums) for one loss form"""
    model = form_model(variant, nc, form).train()
    x = synth.synth_images(batch, size, seed=11)
    targets = synth.synth_targets(batch, size, nc, nmin=nmin, nmax=nmax, seed=5)
    if empty_first:
        a = targets[0]['anns']['det'][0]
        a['boxes'], a['labels'] = a['boxes'][:0], a['labels'][:0]
    losses, _ = model(x, targets, compute_masks=True)
    loss = losses['det']['det_loss'] + losses['det']['mask_loss']
    loss.backward()
    out = {'meta': np.array([batch, size, nc, nmin, nmax]), 'empty_first': np.array(int(empty_first)),
           'loss': npf(losses['det']['det_loss'])}
    out.update(form_entries(form))
    for k, v in losses['det']['loss_items'].items():
        out[f'loss_{k}'] = npf(v)
    sd = model.state_dict()
    for k in STAT_KEYS:
        if k in sd:
            out['stat:' + k] = npf(sd[k])
    params = dict(model.named_parameters())
    for k in GRAD_KEYS:
        if k in params and params[k].numel() <= 40000:
            out['grad:' + k] = npf(params[k].grad)
    names, sums = [], []
    for k, p in params.items():
        if p.grad is None:
            continue
        names.append(k)
        g64 = p.grad.double()
        sums.append([g64.sum().item(), g64.abs().sum().item(), g64.pow(2).sum().sqrt().item()])
    out['gradsum_names'] = np.array(names)
    out['gradsum'] = np.array(sums, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, f'train_{tag}.npz'), **out)
    print('wrote', f'train_{tag}.npz', 'loss', out['loss'], {k: float(out[k].reshape(-1)[0]) for k in out if k.startswith('loss_')})


def gen_trajectory_form(tag, variant, nc, batch, size, steps, nmin, nmax, form, lr=0.01):
    """make_golden.gen_trajectory for one loss form: the reference's losses over `steps` SGD steps on one fixed batch, and the same loop
    with 8 host threads and with every weight perturbed by 1e-6 relative (the band a faithful implementation is held to)"""
    hyp = form_hyp(form)

    def run(threads, perturb=0.0):
        torch.set_num_threads(threads)
        model = form_model(variant, nc, form).train()
        if perturb:
            gen = torch.Generator().manual_seed(123)
            with torch.no_grad():
                for q in model.parameters():
                    q.mul_(1 + perturb * torch.randn(q.shape, generator=gen))
        x = synth.synth_images(batch, size, seed=11)
        targets = synth.synth_targets(batch, size, nc, nmin=nmin, nmax=nmax, seed=5)
        g_bn, g_w, g_b = [], [], []
        for m in model.modules():
            if hasattr(m, 'bias') and isinstance(m.bias, nn.Parameter):
                g_b.append(m.bias)
            if isinstance(m, nn.BatchNorm2d):
                g_bn.append(m.weight)
            elif hasattr(m, 'weight') and isinstance(m.weight, nn.Parameter):
                g_w.append(m.weight)
        opt = torch.optim.SGD(g_bn, lr=lr, momentum=hyp['momentum'], nesterov=True)
        opt.add_param_group({'params': g_w, 'weight_decay': hyp['weight_decay']})
        opt.add_param_group({'params': g_b})
        losses = []
        for _ in range(steps):
            out, _ = model(x, targets, compute_masks=True)
            loss = out['det']['det_loss']
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            losses.append(float(loss.detach()))
        return np.array(losses, dtype=np.float64)

    losses, l8, lp = run(1), run(8), run(1, 1e-6)
    torch.set_num_threads(1)
    np.savez_compressed(os.path.join(HERE, f'trajectory_{tag}.npz'), meta=np.array([batch, size, nc, nmin, nmax, steps]), lr=np.array(lr),
                        weight_decay=np.array(hyp['weight_decay']), momentum=np.array(hyp['momentum']), losses=losses, losses_8_threads=l8,
                        losses_perturbed_1e6=lp, **form_entries(form))
    print('wrote', f'trajectory_{tag}.npz', [round(v, 4) for v in losses], 'own deviation: 8 threads', float((np.abs(l8 - losses) / losses).max()),
          'weights * (1 + 1e-6 n)', float((np.abs(lp - losses) / losses).max()))


def gen_keys_focal():
    out = {}
    for v, nc, form in [('n', 2, FORMS['focal']), ('s', 3, FORMS['focal_s'])]:
        sd = form_model(v, nc, form).state_dict()
        out[f'{v}_keys'] = np.array(list(sd.keys()))
        out[f'{v}_shapes'] = np.array([','.join(map(str, t.shape)) for t in sd.values()])
        out[f'{v}_nc'] = np.array(nc)
    out['n_form'] = np.array('focal')
    out['s_form'] = np.array('focal_s')
    np.savez_compressed(os.path.join(HERE, 'keys_focal.npz'), **out)
    print('wrote keys_focal.npz', len(out['n_keys']), len(out['s_keys']))


def main():
    assert os.path.isdir(mg.REF), 'the reference is only mounted in the build container'
    mg.install_shims()
    torch.set_num_threads(1)
    gen_keys_focal()
    gen_train_form('focal_n_64_ragged', 'n', 2, 2, 64, 3, 8, FORMS['focal'], empty_first=True)
    gen_train_form('focal_s_128', 's', 3, 2, 128, 10, 30, FORMS['focal_s'])
    gen_train_form('iou_target_n_256', 'n', 2, 2, 256, 60, 200, FORMS['iou_target'])
    gen_train_form('clspw_n_64', 'n', 2, 2, 64, 3, 8, FORMS['clspw'])
    gen_trajectory_form('focal_n_128', 'n', 2, 4, 128, 10, 4, 12, FORMS['focal'])


if __name__ == '__main__':
    main()
