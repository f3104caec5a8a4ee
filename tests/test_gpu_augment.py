"""Device augmentation (csrc/augment.hip) on the MI355X against its CPU restatement (tests/augment_ref.py): hdy_augment_tiles_u8 and
hdy_augment_boxes bit for bit, overflow, repeats, poisoned outputs, the DeviceTiles loader end to end and train.py --tile-bank."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_ref as ref  # noqa: E402
from hd_yolo_amd import augment, ops, synth  # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
POISON = {'A': 0, 'B': -1, 'C': 0x7F}          # byte patterns of tests/test_gpu_scratch.py: 0x00.., 0xFF.., 0x7F7F..


def make_hyp(k, patch, size, perspective=0.0, **kw):
    hyp = dict(degrees=25.0, translate=0.15, scale=0.4, shear=8.0, perspective=perspective, hsv_h=0.05, hsv_s=0.7, hsv_v=0.4, fliplr=0.5,
               flipud=0.5, transpose=0.5, cval=114, k_mosaic=k, patch_size=patch, img_size=size)
    hyp.update(kw)
    return hyp


def make_case(seed, n, tile, k, patch, size, B, channels=3, perspective=0.0, odd_pitch=False):
    """bank (numpy + device view), drawn parameters with every flip combination and HSV on / off inside every image, packed tables"""
    rng = np.random.default_rng(seed)
    bank = synth.synth_tile_bank(n, tile, 3, seed=seed, nmin=6, nmax=14)
    tiles = bank.tiles
    if channels == 4:
        tiles = np.concatenate([tiles, rng.integers(0, 256, tiles.shape[:3] + (1,), dtype=np.uint8)], -1)
    hyp = make_hyp(k, patch, size, perspective)
    p = augment.draw_params(rng, hyp, B, n)
    cells = np.arange(B * k * k).reshape(B, k * k)
    combo = (cells + np.arange(B)[:, None]) % 8                  # all eight flip combinations, different ones inside an image
    p['hflip'], p['vflip'], p['transpose'] = (combo & 1) > 0, (combo & 2) > 0, (combo & 4) > 0
    p['hsv'] = (cells % 2 == 0) if k > 1 else (np.arange(B)[:, None] % 2 == 0)
    tab = augment.cell_tables(p, (tile, tile))
    if odd_pitch:                                                # a cropped view of a larger allocation with an odd row pitch and tile stride
        pitch = tile * channels + 7 + (tile * channels) % 2
        stride = tile * pitch + 13
        flat = torch.from_numpy(rng.integers(0, 256, n * stride + 64, dtype=np.uint8))
        host = torch.as_strided(flat, (n, tile, tile, channels), (stride, pitch, channels, 1), 5)
        host.copy_(torch.from_numpy(tiles))
        d_tiles = torch.as_strided(flat.to(DEV), (n, tile, tile, channels), (stride, pitch, channels, 1), 5)
        assert pitch % 2 == 1
    else:
        d_tiles = torch.from_numpy(tiles).to(DEV)
    return {'bank': bank, 'tiles': tiles, 'd_tiles': d_tiles, 'hyp': hyp, 'tab': tab, 'k': k, 'patch': patch, 'size': size, 'B': B, 'cval': 114}


def upload(tab):
    return torch.from_numpy(tab.cells.copy()).to(DEV), torch.from_numpy(tab.crop.copy()).to(DEV)


def expected_image(case, dtype):
    p = ref.augment_tiles_ref(case['tiles'], case['tab'].cells, case['tab'].crop, case['patch'], case['k'], case['size'], case['cval'])
    return torch.from_numpy(ref.u8_table()[p]).to(dtype)


def bits(t):
    return t.contiguous().view(INT_VIEW[t.dtype]).cpu()


IMAGE_CASES = {
    # id: (n, tile, k, patch, size, B, channels, perspective, odd_pitch, dtype)
    'bf16_rgb_k2_patch_ne_tile': (5, 40, 2, 48, 70, 8, 3, 0.0, False, torch.bfloat16),
    'fp32_rgba_k2_odd_pitch_view': (4, 36, 2, 36, 54, 8, 4, 0.0, True, torch.float32),
    'bf16_rgb_k3_perspective_odd_size': (6, 32, 3, 40, 75, 8, 3, 0.002, True, torch.bfloat16),
    'fp32_rgb_k1_full_canvas': (3, 44, 1, 44, 44, 8, 3, 0.001, False, torch.float32),
    'bf16_rgba_k1_crop': (3, 64, 1, 80, 50, 8, 4, 0.0, False, torch.bfloat16),
}


@pytest.mark.parametrize('name', sorted(IMAGE_CASES))
def test_augment_tiles_matches_the_restatement_bit_for_bit(name):
    n, tile, k, patch, size, B, ch, persp, odd, dtype = IMAGE_CASES[name]
    case = make_case(11, n, tile, k, patch, size, B, ch, persp, odd)
    cells, crop = upload(case['tab'])
    want = expected_image(case, dtype)
    first = None
    for pat in 'ABC':                                            # poisoned output before the call: every element is written
        out = torch.empty((B, 3, size, size), dtype=dtype, device=DEV)
        out.view(torch.uint8).fill_(POISON[pat] & 255)
        ops.augment_tiles(case['d_tiles'], cells, crop, out, patch, k, case['cval'])
        got = bits(out)
        assert torch.equal(got, bits(want)), f'{name}: {(got != bits(want)).sum().item()} of {got.numel()} elements differ (pattern {pat})'
        first = got if first is None else first
        assert torch.equal(got, first)
    want_u8 = ref.augment_tiles_ref(case['tiles'], case['tab'].cells, case['tab'].crop, patch, k, size, case['cval'])
    assert (want_u8 != case['cval']).mean() > 0.3, 'the case must show source pixels, not only the border'


def test_augment_tiles_table_content_cannot_reach_outside_the_bank():
    """a source index outside the bank reads as the border value; a crop offset outside the mosaic gives an image of the border value"""
    case = make_case(3, 3, 32, 2, 32, 40, 4)
    tab = case['tab']
    w = tab.cells[:, :96].view(np.int32)
    w[1, 0], w[2, 0], w[5, 0] = -1, 3, 2 ** 30
    tab.crop[3] = (25, 0)                                        # 25 + 40 > 2 * 32
    tab.crop[2] = (-1, 3)
    cells, crop = upload(tab)
    out = torch.empty((4, 3, 40, 40), dtype=torch.float32, device=DEV)
    ops.augment_tiles(case['d_tiles'], cells, crop, out, 32, 2, 114)
    want = expected_image(case, torch.float32)
    assert torch.equal(bits(out), bits(want))
    assert (out[3] == out[3, 0, 0, 0]).all() and (out[2] == out[3, 0, 0, 0]).all()


def run_boxes(case, cap, pad=0, pattern=None):
    bank = case['bank']
    cells, crop = upload(case['tab'])
    B = case['B']
    d = {'boxes': torch.zeros((cap + pad, 4), device=DEV), 'labels': torch.zeros((cap + pad,), dtype=torch.int64, device=DEV),
         'img': torch.zeros((cap + pad,), device=DEV), 'counts': torch.zeros((B,), dtype=torch.int32, device=DEV),
         'overflow': torch.zeros((1,), dtype=torch.int32, device=DEV)}
    if pattern is not None:
        for t in d.values():
            t.view(torch.uint8).fill_(POISON[pattern] & 255)
    ops.augment_boxes(torch.from_numpy(bank.boxes).to(DEV), torch.from_numpy(bank.labels).to(DEV), torch.from_numpy(bank.offsets).to(DEV),
                      len(bank.boxes), cells, crop, case['patch'], case['k'], case['size'], d['boxes'][:cap], d['labels'][:cap], d['img'][:cap],
                      d['counts'], d['overflow'])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


@pytest.mark.parametrize('name', sorted(IMAGE_CASES))
def test_augment_boxes_match_the_fp32_restatement(name):
    n, tile, k, patch, size, B, ch, persp, odd, _ = IMAGE_CASES[name]
    case = make_case(11, n, tile, k, patch, size, B, ch, persp, odd)
    bank = case['bank']
    wb, wl, wi, wc = ref.augment_boxes_ref(bank.boxes, bank.labels, bank.offsets, case['tab'].cells, case['tab'].crop, patch, k, size)
    T = len(wb)
    assert T > 0 and T < int(np.diff(bank.offsets)[ref.parse_cells(case['tab'].cells)['src']].sum()), 'some boxes kept, some dropped'
    first = None
    for pat in 'ABC':
        got = run_boxes(case, T + 5, pattern=pat)
        assert got['overflow'].item() == 0
        assert torch.equal(got['counts'], torch.from_numpy(wc))
        assert torch.equal(got['boxes'][:T].view(torch.int32), torch.from_numpy(wb).view(torch.int32)), name
        assert torch.equal(got['labels'][:T], torch.from_numpy(wl)) and torch.equal(got['img'][:T], torch.from_numpy(wi))
        assert (got['boxes'][T:].view(torch.uint8) == (POISON[pat] & 255)).all(), 'rows beyond the kept ones are not written'
        cur = {k_: v[:T] if k_ in ('boxes', 'labels', 'img') else v for k_, v in got.items()}
        first = cur if first is None else first
        assert all(torch.equal(cur[k_].view(torch.uint8), first[k_].view(torch.uint8)) for k_ in cur)


def test_augment_boxes_overflow_sets_the_flag_and_writes_nothing_past_cap():
    case = make_case(11, 5, 40, 2, 48, 70, 8)
    bank = case['bank']
    wb, wl, wi, wc = ref.augment_boxes_ref(bank.boxes, bank.labels, bank.offsets, case['tab'].cells, case['tab'].crop, 48, 2, 70)
    cap = len(wb) // 2
    assert cap > 4
    for pat in 'ABC':
        got = run_boxes(case, cap, pad=64, pattern=pat)
        assert got['overflow'].item() == 1
        assert torch.equal(got['counts'], torch.from_numpy(wc)), 'the counts are the true ones'
        assert torch.equal(got['boxes'][:cap].view(torch.int32), torch.from_numpy(wb[:cap]).view(torch.int32))
        assert torch.equal(got['labels'][:cap], torch.from_numpy(wl[:cap])) and torch.equal(got['img'][:cap], torch.from_numpy(wi[:cap]))
        for key in ('boxes', 'labels', 'img'):
            assert (got[key][cap:].contiguous().view(torch.uint8) == (POISON[pat] & 255)).all(), f'{key}: written past cap (pattern {pat})'
    exact = run_boxes(case, len(wb), pad=8, pattern='B')
    assert exact['overflow'].item() == 0 and torch.equal(exact['boxes'][:len(wb)].view(torch.int32), torch.from_numpy(wb).view(torch.int32))


def test_two_runs_give_identical_bits_at_flagship_shape_subset():
    """a larger batch (64 images of 160 px from 2 x 2 cells of 96 px), twice, with other work on the stream in between"""
    case = make_case(5, 12, 96, 2, 96, 160, 64)
    cells, crop = upload(case['tab'])
    outs = []
    for rep in range(2):
        out = torch.empty((64, 3, 160, 160), dtype=torch.bfloat16, device=DEV)
        ops.augment_tiles(case['d_tiles'], cells, crop, out, 96, 2, 114)
        outs.append(bits(out))
        torch.randn(1 << 20, device=DEV).sum()
    assert torch.equal(outs[0], outs[1])
    a, b = run_boxes(case, 64 * 4 * 14), run_boxes(case, 64 * 4 * 14)
    assert all(torch.equal(a[k], b[k]) for k in a) and a['counts'].sum() > 0
    assert torch.equal(outs[0][:4], bits(expected_image({**case, 'B': 4, 'tab': sub_tables(case['tab'], 4)}, torch.bfloat16)))


def sub_tables(tab, B):
    k2 = tab.k * tab.k
    packed = np.concatenate([tab.cells[:B * k2].reshape(-1), tab.crop[:B].reshape(-1).view(np.uint8)])
    return augment.CellTables(packed, B, tab.k, tab.M[:B], tab.Minv[:B])


# ---------------------------------------------------------------------------------------------------------------- DeviceTiles end to end
def loader_for(steps=3, B=4, size=64, seed=0, **kw):
    from metayolo.datasets import DeviceTiles
    bank = synth.synth_tile_bank(6, 96, 2, seed=1)
    hyp = make_hyp(2, 80, size, perspective=0.0005)
    return DeviceTiles(bank, hyp, B, steps, rank=0, seed=seed, device=DEV, **kw), bank, hyp


def collect(loader):
    out = []
    for imgs, targets in loader:
        out.append((torch.stack(list(imgs)).clone(), [(t['anns']['det'][0]['boxes'].clone(), t['anns']['det'][0]['labels'].clone()) for t in targets]))
    return out


def test_device_tiles_epochs_are_reproducible_and_match_the_restatement():
    loader, bank, hyp = loader_for()
    loader.set_epoch(0)
    e0 = collect(loader)
    loader.set_epoch(1)
    e1 = collect(loader)
    loader.set_epoch(0)
    again = collect(loader)
    assert loader.d2h_copies == 9, 'one device-to-host copy (the row counts) per batch'
    assert len(e0) == 3
    for (xa, ta), (xb, tb) in zip(e0, again):
        assert torch.equal(bits(xa), bits(xb))
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(ta, tb))
    assert not torch.equal(bits(e0[0][0]), bits(e1[0][0])) and not torch.equal(bits(e0[0][0]), bits(e0[1][0]))
    # batch 1 of epoch 0 from the same draw on the CPU
    p = augment.draw_params(augment.step_rng(0, 0, 0, 1), hyp, 4, bank.n)
    tab = augment.cell_tables(p, (96, 96))
    want = torch.from_numpy(ref.u8_table()[ref.augment_tiles_ref(bank.tiles, tab.cells, tab.crop, 80, 2, 64, 114)]).to(torch.bfloat16)
    assert torch.equal(bits(e0[1][0]), bits(want))
    wb, wl, wi, wc = ref.augment_boxes_ref(bank.boxes, bank.labels, bank.offsets, tab.cells, tab.crop, 80, 2, 64)
    assert [len(t[0]) for t in e0[1][1]] == wc.tolist()
    assert torch.equal(torch.cat([t[0] for t in e0[1][1]]).cpu().view(torch.int32), torch.from_numpy(wb).view(torch.int32))
    assert torch.equal(torch.cat([t[1] for t in e0[1][1]]).cpu(), torch.from_numpy(wl))
    from metayolo.datasets import DeviceTiles
    other_rank = collect(DeviceTiles(bank, hyp, 4, 1, rank=1, seed=0, device=DEV))
    assert not torch.equal(bits(other_rank[0][0]), bits(e0[0][0]))


def test_device_tiles_batch_has_the_target_schema_and_trains():
    from metayolo.models.yolo import Model
    loader, bank, hyp = loader_for(steps=2)
    cfg, mhyp = synth.make_cfg('n', 2), synth.make_hyp(conf_thres=0.05)
    model = Model(cfg, mhyp)
    model.load_state_dict(synth.synth_state_dict(synth.shapes_of(model), seed=0), strict=False)
    model = model.to(DEV).train()
    it = iter(loader)
    imgs, targets = next(it)
    assert len(imgs) == 4 and imgs[0].shape == (3, 64, 64) and imgs[0].dtype == torch.bfloat16 and imgs[0].is_cuda
    plain_like = synth.synth_targets(4, 64, 2, nmin=2, nmax=3, seed=0)
    total = 0
    for t, s in zip(targets, plain_like):
        assert set(t) == set(s) and set(t['anns']) == {'det'} and set(t['anns']['det'][0]) == set(s['anns']['det'][0])
        a = t['anns']['det'][0]
        assert a['boxes'].is_cuda and a['boxes'].dtype == torch.float32 and a['boxes'].shape[1] == 4 and a['labels'].dtype == torch.int64
        assert t['size'].tolist() == [64, 64] and a['labels'].shape[0] == a['boxes'].shape[0]
        if len(a['boxes']):
            assert a['boxes'].min() >= 0 and a['boxes'].max() <= 1 and a['labels'].min() >= 1 and a['labels'].max() <= 2
            assert ((a['boxes'][:, 2:] - a['boxes'][:, :2]) * 64 > 10 - 1e-3).all()
        total += len(a['boxes'])
    assert total > 0
    x = torch.stack(list(imgs))
    plain = tuple({'image_id': t['image_id'], 'size': t['size'],
                   'anns': {'det': [{'size': t['size'], 'boxes': t['anns']['det'][0]['boxes'].cpu().clone(),
                                     'labels': t['anns']['det'][0]['labels'].cpu().clone()}]}} for t in targets)
    losses, _ = model(x, targets)
    loss = losses['det']['det_loss']
    assert torch.isfinite(loss).all()
    loss.backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    losses2, _ = model(x.float().cpu().to(DEV).to(torch.bfloat16), plain)
    assert torch.equal(loss.detach().view(torch.int32).cpu(), losses2['det']['det_loss'].detach().view(torch.int32).cpu()), \
        (loss.item(), losses2['det']['det_loss'].item())
    next(it)
    assert loader.d2h_copies == 2


def test_device_tiles_refuses_what_it_does_not_implement():
    from metayolo.datasets import DeviceTiles
    bank = synth.synth_tile_bank(2, 32, 2, seed=0, nmin=2, nmax=3)
    good = make_hyp(1, 32, 32)
    for bad, exc in (({'color_aug': 'jitter'}, ValueError), ({'keep_res': 0.5}, ValueError), ({'img_size': 80}, ValueError),
                     ({'k_mosaic': 9}, ValueError)):
        with pytest.raises(exc):
            DeviceTiles(bank, {**good, **bad}, 2, 1, device=DEV)
    missing = dict(good)
    del missing['shear']
    with pytest.raises(KeyError):
        DeviceTiles(bank, missing, 2, 1, device=DEV)
    small = DeviceTiles(bank, make_hyp(1, 32, 32, degrees=0.0, scale=0.0, shear=0.0, translate=0.0), 2, 1, device=DEV, cap=1)
    with pytest.raises(RuntimeError, match='capacity'):
        list(small)


def test_train_py_runs_on_a_tile_bank(tmp_path):
    path = str(tmp_path / 'bank.npz')
    synth.synth_tile_bank(8, 128, 2, seed=3).save(path)
    cmd = [sys.executable, 'train.py', '--variant', 'n', '--nc', '2', '--batch-size', '8', '--imgsz', '128', '--epochs', '1', '--steps-per-epoch', '4',
           '--val-batches', '1', '--project', str(tmp_path), '--name', 'bank', '--exist-ok', '--tile-bank', path, '--k-mosaic', '2', '--patch-size', '96',
           '--degrees', '10', '--perspective', '0.0005']
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, YOLOv5_VERBOSE='true'), capture_output=True, text=True, timeout=500)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert 'epochs completed' in p.stdout + p.stderr
    ck = torch.load(tmp_path / 'bank' / 'weights' / 'last.pt', map_location='cpu')
    assert all(torch.isfinite(v).all() for v in ck['model'].values() if v.dtype.is_floating_point)
