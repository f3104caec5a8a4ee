"""CPU checks of the other DetLoss forms on the fused loss (csrc/loss.hip): which criteria Detect.fused_loss_ok() routes to it, the
state-dict surface of focal models against the reference (keys_focal.npz), and hdy_det_loss_ex's argument checks (before any device work)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from hd_yolo_amd import _lib, build, synth

FORMS = {
    'bce': {},
    'focal': {'fl_gamma': 1.5},
    'focal_s': {'fl_gamma': 2.0, 'label_smoothing': 0.1, 'cls_pw': [1.0, 2.0, 0.5], 'obj_pw': 0.7, 'cls_cw': [1.0, 0.5, 2.0]},
    'iou_target': {'fl_gamma': 1.5, 'gr': 0.5, 'sort_obj_iou': True},
    'clspw': {'cls_pw': [1.5, 0.5]},
}


def model_for(form, variant='n', nc=None):
    from metayolo.models.yolo import Model
    nc = nc or (3 if form == 'focal_s' else 2)
    opts = FORMS[form]
    hyp = synth.make_hyp()
    hyp['det'].update({k: v for k, v in opts.items() if k not in ('gr', 'sort_obj_iou')})
    model = Model(synth.make_cfg(variant, nc), hyp)
    dl = model.headers['det'].det_loss
    dl.gr, dl.sort_obj_iou = opts.get('gr', 1.0), opts.get('sort_obj_iou', False)
    return model


def head(model):
    return model.headers['det']


@pytest.fixture(autouse=True)
def fused_on(monkeypatch):
    monkeypatch.delenv('HDY_FUSED_LOSS', raising=False)


@pytest.mark.parametrize('form', list(FORMS))
def test_fused_loss_covers_the_loss_forms(form):
    h = head(model_for(form))
    assert h.fused_loss_ok()
    dl = h.det_loss
    for gr in (0.0, 0.3, 1.0, 1.5):
        dl.gr = gr
        assert h.fused_loss_ok(), gr
    dl.sort_obj_iou = not dl.sort_obj_iou
    assert h.fused_loss_ok()


def test_fused_loss_rejects_what_it_does_not_compute(monkeypatch):
    from metayolo.models.loss import FocalLoss
    h = head(model_for('focal'))
    dl = h.det_loss
    assert h.fused_loss_ok()
    monkeypatch.setenv('HDY_FUSED_LOSS', '0')
    assert not h.fused_loss_ok()
    monkeypatch.delenv('HDY_FUSED_LOSS')
    dl.gr = float('nan')
    assert not h.fused_loss_ok()
    dl.gr = 1.0
    dl.autobalance = True
    assert not h.fused_loss_ok()
    dl.autobalance = False
    cls_focal, obj_focal = dl.BCEcls, dl.BCEobj
    dl.BCEobj = obj_focal.loss_fcn                       # focal class term, BCE objectness
    assert not h.fused_loss_ok()
    dl.BCEobj, dl.BCEcls = obj_focal, cls_focal.loss_fcn   # BCE class term, focal objectness
    assert not h.fused_loss_ok()
    dl.BCEcls = cls_focal
    obj_focal.gamma = 2.0                                # unequal gamma
    assert not h.fused_loss_ok()
    obj_focal.gamma = 1.5
    obj_focal.alpha = 0.5                                # unequal alpha
    assert not h.fused_loss_ok()
    obj_focal.alpha = 0.25
    assert h.fused_loss_ok()
    dl.BCEobj = FocalLoss(torch.nn.MSELoss(), 1.5)       # another criterion class
    assert not h.fused_loss_ok()
    dl.BCEobj = obj_focal
    dl.BCEcls.loss_fcn.loss_fn = torch.nn.BCELoss(reduction='none')
    assert not h.fused_loss_ok()


def test_fused_loss_rejects_more_than_128_classes():
    h = head(model_for('focal', nc=129))
    assert not h.fused_loss_ok()


def test_focal_model_state_dict_keys_match_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, 'keys_focal.npz'))
    for v in ('n', 's'):
        sd = model_for(str(g[f'{v}_form']), v, int(g[f'{v}_nc'])).state_dict()
        assert list(sd.keys()) == [str(k) for k in g[f'{v}_keys']], v
        assert [','.join(map(str, t.shape)) for t in sd.values()] == [str(s) for s in g[f'{v}_shapes']], v
    assert any(k.endswith('det_loss.BCEobj.loss_fcn.pos_weight') for k in g['n_keys'])


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize('gamma,alpha,gr,what', [
    (-0.5, 0.25, 1.0, b'fl_gamma'), (math.nan, 0.25, 1.0, b'fl_gamma'), (math.inf, 0.25, 1.0, b'fl_gamma'),
    (1.5, math.nan, 1.0, b'fl_alpha'), (1.5, math.inf, 1.0, b'fl_alpha'),
    (1.5, 0.25, math.nan, b': gr must'), (0.0, 0.25, -math.inf, b': gr must')])
def test_det_loss_ex_rejects_bad_form_parameters(lib, gamma, alpha, gr, what):
    """a status and a message before any device work: every pointer is null here, and no GPU is needed"""
    nl, na, nc = 3, 3, 2
    ny, nx = (ctypes.c_int * nl)(8, 4, 2), (ctypes.c_int * nl)(8, 4, 2)
    rc = lib.hdy_det_loss_ex(None, 28, None, 28, _lib.F32, ny, nx, nl, 1, na, nc, None, None, None, None, 0, None, None,
                             1.0, 4.0, 0.0, 0.05, 1.0, 0.5, gamma, alpha, gr, 0, None, None, 0, None)
    assert rc == _lib.EINVAL
    msg = lib.hdy_last_error()
    assert what in msg, msg
