"""Instance masks through the device augmentation (csrc/augment_masks.hip) on the MI355X against their CPU restatement
(tests/augment_mask_ref.py, which scans the whole canvas): extents records, boxes, labels, image indices, counts, out_ref, total and the
28 x 28 targets bit for bit; the unmasked path against hdy_augment_boxes; overflow; hostile table content; repeats and poisoned workspaces;
the DeviceTiles loader with masks end to end and train.py --masks --tile-bank."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_mask_cases as cases  # noqa: E402
import augment_mask_ref as mref  # noqa: E402
import augment_ref as ref  # noqa: E402
from hd_yolo_amd import augment, ops, synth  # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256                                     # sentinel bytes in front of and behind every output buffer
P, K, S = cases.PATCH, cases.K, cases.SIZE


class Guarded:
    """an output buffer between two sentinel zones, everything filled with one byte"""

    def __init__(self, shape, dtype, fill):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.fill = fill
        self.flat = torch.full((2 * GUARD + (self.nbytes + 15) // 16 * 16,), fill, dtype=torch.uint8, device=DEV)
        self.t = self.flat[GUARD:GUARD + self.nbytes].view(dtype).view(shape)

    def guards_intact(self):
        return bool((self.flat[:GUARD] == self.fill).all()) and bool((self.flat[GUARD + self.nbytes:] == self.fill).all())

    def untouched(self, first_row):
        """rows from first_row on still hold the fill byte"""
        return bool((self.t[first_row:].contiguous().view(torch.uint8) == self.fill).all())


def device_bank(bank, offsets=None):
    d = {'boxes': torch.from_numpy(bank.boxes).to(DEV), 'labels': torch.from_numpy(bank.labels).to(DEV),
         'offsets': torch.from_numpy(np.asarray(bank.offsets if offsets is None else offsets, np.int64)).to(DEV), 'n_boxes': len(bank.boxes)}
    if bank.instances is not None:
        d['inst'] = torch.from_numpy(bank.instances.view(np.int16)).to(DEV)
        d['has'] = torch.from_numpy(bank.has_mask).to(DEV)
    return d


def run(bank, cells, crop, cap, pitch, fill=0xA5, ws_fill=0x5A, offsets=None, B=cases.B, patch=P, k=K, size=S):
    """the three launches into guarded, sentinel-filled buffers -> (dict of CPU arrays, dict of the Guarded buffers)"""
    d = device_bank(bank, offsets)
    n_cells = len(cells)
    dc, dr = torch.from_numpy(np.ascontiguousarray(cells)).to(DEV), torch.from_numpy(np.ascontiguousarray(crop, np.int32)).to(DEV)
    g = {'ws': Guarded((ops.augment_mask_workspace_bytes(n_cells, pitch),), torch.uint8, ws_fill), 'boxes': Guarded((cap, 4), torch.float32, fill),
         'labels': Guarded((cap,), torch.int64, fill), 'img': Guarded((cap,), torch.float32, fill), 'ref': Guarded((cap, 2), torch.int32, fill),
         'counts': Guarded((B + 1,), torch.int32, fill), 'total': Guarded((1,), torch.int32, fill),
         'masks': Guarded((cap, 28, 28), torch.float32, fill)}
    ops.augment_mask_extents(d['inst'], d['boxes'], d['has'], d['offsets'], d['n_boxes'], dc, dr, patch, k, size, g['ws'].t, pitch)
    ops.augment_boxes_masks(d['boxes'], d['labels'], d['has'], d['offsets'], d['n_boxes'], dc, dr, patch, k, size, g['ws'].t, pitch, g['boxes'].t,
                            g['labels'].t, g['img'].t, g['ref'].t, g['counts'].t[:B], g['counts'].t[B:], g['total'].t)
    ops.augment_mask_targets(d['inst'], d['has'], d['offsets'], d['n_boxes'], dc, dr, patch, k, size, g['ws'].t, pitch, g['boxes'].t, g['ref'].t,
                             g['total'].t, g['masks'].t)
    torch.cuda.synchronize()
    out = {key: v.t.cpu().numpy() for key, v in g.items()}
    out['rec'] = out.pop('ws').view(np.int32).reshape(n_cells, pitch, 8)
    return out, g


def assert_equals_restatement(got, g, rec, written, rows, cap, fill, ws_fill, what):
    """every element: records (written ones; the others keep the workspace's fill), rows, counts, total; nothing behind the rows; guards"""
    T = len(rows['boxes'])
    n = min(T, cap)
    assert np.array_equal(got['rec'][written], rec[written]), f'{what}: extents records'
    assert (got['rec'][~written].view(np.uint8) == ws_fill).all(), f'{what}: a record that is no candidate was written'
    assert got['total'].tolist() == [n] and got['counts'][-1] == (1 if T > cap else 0), what
    assert np.array_equal(got['counts'][:-1], rows['counts']), f'{what}: counts'
    assert np.array_equal(got['boxes'][:n].view(np.int32), rows['boxes'][:n].view(np.int32)), f'{what}: boxes'
    assert np.array_equal(got['labels'][:n], rows['labels'][:n]) and np.array_equal(got['img'][:n], rows['img'][:n]), f'{what}: labels / image'
    assert np.array_equal(got['ref'][:n], rows['ref'][:n]), f'{what}: out_ref'
    diff = got['masks'][:n].view(np.int32) != rows['masks'][:n].view(np.int32)
    assert not diff.any(), f'{what}: {int(diff.sum())} mask elements in rows {np.unique(np.nonzero(diff)[0]).tolist()} differ'
    for key in ('boxes', 'labels', 'img', 'ref', 'masks'):
        assert g[key].untouched(n), f'{what}: {key} written past row {n}'
    for key, v in g.items():
        assert v.guards_intact(), f'{what}: bytes around {key} were written'


@pytest.mark.parametrize('name', sorted(cases.PARITY_CASES))
def test_masks_match_the_restatement_bit_for_bit(name):
    case = cases.parity_case(name)
    rows = case['rows']
    T = len(rows['boxes'])
    got, g = run(case['bank'], case['tab'].cells, case['tab'].crop, T + 3, case['pitch'])
    assert_equals_restatement(got, g, case['rec'], case['written'], rows, T + 3, 0xA5, 0x5A, name)
    st = case['stats']
    assert st['nonzero_targets'] >= 10 and st['kept_at_001_not_010'] >= 1 and st['unmasked_kept'] >= 1 and st['drop_final'] >= 1
    # over all cases (the restatement alone; CPU twin: test_augment_masks_host.test_the_parity_cases_are_not_vacuous)
    tot = cases.total_stats()
    assert tot['nonzero_targets'] >= 20 and tot['zeroed_by_25'] >= 1 and tot['unmasked_kept'] >= 1 and tot['kept_at_001_not_010'] >= 1
    assert tot['drop_candidate'] >= 1 and tot['drop_final'] >= 1


def test_an_unmasked_bank_equals_augment_boxes_bit_for_bit():
    case = cases.parity_case('persp_strong')
    full, tab = case['bank'], case['tab']
    bank = augment.TileBank(full.tiles, full.boxes, full.labels, full.offsets, np.full_like(full.instances, 0xFFFF))
    cap = 40
    got, g = run(bank, tab.cells, tab.crop, cap, case['pitch'])
    d = device_bank(bank)
    dc, dr = torch.from_numpy(tab.cells.copy()).to(DEV), torch.from_numpy(tab.crop.copy()).to(DEV)
    ob, ol, oi = torch.zeros((cap, 4), device=DEV), torch.zeros((cap,), dtype=torch.int64, device=DEV), torch.zeros((cap,), device=DEV)
    cnt = torch.zeros((cases.B + 1,), dtype=torch.int32, device=DEV)
    ops.augment_boxes(d['boxes'], d['labels'], d['offsets'], d['n_boxes'], dc, dr, P, K, S, ob, ol, oi, cnt[:cases.B], cnt[cases.B:])
    n = int(cnt[:cases.B].sum())
    assert 0 < n < cap and got['total'].tolist() == [n]
    assert np.array_equal(got['counts'], cnt.cpu().numpy())
    assert np.array_equal(got['boxes'][:n].view(np.int32), ob[:n].cpu().numpy().view(np.int32))
    assert np.array_equal(got['labels'][:n], ol[:n].cpu().numpy()) and np.array_equal(got['img'][:n], oi[:n].cpu().numpy())
    assert not got['masks'][:n].any() and g['masks'].untouched(n)
    assert all(v.guards_intact() for v in g.values())


def test_overflow_sets_the_flag_and_writes_nothing_past_cap():
    case = cases.parity_case('affine_mild')
    T = len(case['rows']['boxes'])
    cap = T // 2
    assert cap > 4
    for fill in (0xA5, 0x00, 0xFF):
        got, g = run(case['bank'], case['tab'].cells, case['tab'].crop, cap, case['pitch'], fill=fill)
        assert got['counts'][-1] == 1 and got['total'].tolist() == [cap]
        assert_equals_restatement(got, g, case['rec'], case['written'], case['rows'], cap, fill, 0x5A, f'overflow fill {fill:#x}')
    got, g = run(case['bank'], case['tab'].cells, case['tab'].crop, T, case['pitch'])
    assert got['counts'][-1] == 0 and got['total'].tolist() == [T]
    assert_equals_restatement(got, g, case['rec'], case['written'], case['rows'], T, 0xA5, 0x5A, 'cap == kept')


@pytest.mark.parametrize('bad_offsets', [None, (-1, 3, 7, 9, 8), (0, 3, 7, 9, 99)], ids=['table', 'offsets_negative_decreasing', 'offsets_beyond'])
def test_table_content_cannot_reach_outside_the_bank_or_the_map(bad_offsets):
    """source index -1 / n / 2^30, crop offsets out of range, offsets rows negative, decreasing or beyond M: such cells own nothing; what the
    kernels write is the restatement's and the sentinels around every buffer are intact (nothing here can fault: every index is checked)"""
    case = cases.parity_case('affine_strong')
    bank = case['bank']
    cells, crop = case['tab'].cells.copy(), case['tab'].crop.copy()
    w = cells[:, :96].view(np.int32)
    bad_cells = set()
    if bad_offsets is None:
        w[1, 0], w[2, 0], w[5, 0] = -1, bank.n, 2 ** 30
        crop[2] = (33, 0)                                        # 33 + 64 > 2 * 48
        bad_cells = {1, 2, 5, 8, 9, 10, 11}
        offsets = bank.offsets
    else:
        assert bank.offsets.tolist() == [0, 3, 7, 9, 15]
        offsets = np.asarray(bad_offsets, np.int64)
        bad_tiles = {0, 3} if bad_offsets[0] < 0 else {3}
        bad_cells = {ci for ci in range(len(cells)) if int(w[ci, 0]) in bad_tiles}
        assert 0 < len(bad_cells) < len(cells)
    pitch = case['pitch']
    rec, written = mref.mask_extents_ref(bank.instances, bank.has_mask, offsets, len(bank.boxes), cells, crop, P, K, S, pitch)
    rows = mref.boxes_masks_ref(bank.boxes, bank.labels, bank.has_mask, offsets, cells, crop, P, K, S, rec, pitch)
    rows['masks'] = mref.mask_targets_ref(bank.instances, cells, crop, P, K, S, rec, rows)
    T = len(rows['boxes'])
    assert T > 0 and not (set(rows['ref'][:, 0].tolist()) & bad_cells) and not written[sorted(bad_cells)].any()
    got, g = run(bank, cells, crop, T + 2, pitch, offsets=offsets)
    assert_equals_restatement(got, g, rec, written, rows, T + 2, 0xA5, 0x5A, 'hostile table')
    if bad_offsets is None:
        assert got['counts'][2] == 0


def test_two_runs_give_identical_bits_and_a_poisoned_workspace_changes_nothing():
    case = cases.parity_case('persp_strong')
    T = len(case['rows']['boxes'])
    outs = [run(case['bank'], case['tab'].cells, case['tab'].crop, T + 1, case['pitch'], fill=f, ws_fill=wf)[0]
            for f, wf in ((0xA5, 0x5A), (0xA5, 0x5A), (0x00, 0xFF), (0xFF, 0x00), (0x7F, 0x7F))]
    written = case['written']
    for o in outs[1:]:
        assert np.array_equal(o['rec'][written], outs[0]['rec'][written])
        for key in ('boxes', 'labels', 'img', 'ref', 'masks'):
            assert np.array_equal(o[key][:T].view(np.uint8), outs[0][key][:T].view(np.uint8)), key
        assert np.array_equal(o['counts'], outs[0]['counts']) and np.array_equal(o['total'], outs[0]['total'])
    assert np.array_equal(outs[0]['masks'][:T].view(np.int32), case['rows']['masks'].view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- DeviceTiles end to end
def masked_loader(steps=2, seed=0, **kw):
    from metayolo.datasets import DeviceTiles
    bank = synth.synth_tile_bank(4, 96, 2, seed=2, nmin=6, nmax=12, instances=True)
    hyp = cases.make_hyp(2, 64, 96, perspective=0.0005, degrees=15.0, shear=4.0, scale=0.3, hsv_h=0.02, hsv_s=0.5, hsv_v=0.3)
    return DeviceTiles(bank, hyp, 4, steps, rank=0, seed=seed, device=DEV, **kw), bank, hyp


def collect(loader):
    out = []
    for imgs, targets in loader:
        a = [t['anns']['det'][0] for t in targets]
        out.append((torch.stack(list(imgs)).clone(), [(x['boxes'].clone(), x['labels'].clone(), x['masks'].clone()) for x in a]))
    return out


def test_device_tiles_masks_are_reproducible_and_match_the_restatement():
    loader, bank, hyp = masked_loader()
    e0 = collect(loader)
    again = collect(loader)
    assert loader.d2h_copies == 4, 'one device-to-host copy (the row counts) per batch'
    for (xa, ta), (xb, tb) in zip(e0, again):
        assert torch.equal(xa.view(torch.int16), xb.view(torch.int16))
        assert all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for a, b in zip(ta, tb) for u, v in zip(a, b))
    for boxes, labels, masks in e0[0][1]:
        assert masks.shape == (len(boxes), 28, 28) and masks.dtype == torch.float32 and masks.is_cuda
        assert len(masks) == 0 or (masks.min() >= 0 and masks.max() <= 1)
    # batch 1 of epoch 0 from the same draw on the CPU
    p = augment.draw_params(augment.step_rng(0, 0, 0, 1), hyp, 4, bank.n)
    tab = augment.cell_tables(p, (96, 96))
    _, _, rows = mref.augment_masks_ref(bank, tab.cells, tab.crop, 64, 2, 96)
    assert [len(t[0]) for t in e0[1][1]] == rows['counts'].tolist() and rows['masked'].sum() >= 8 and rows['masks'].any()
    assert np.array_equal(torch.cat([t[0] for t in e0[1][1]]).cpu().numpy().view(np.int32), rows['boxes'].view(np.int32))
    assert np.array_equal(torch.cat([t[1] for t in e0[1][1]]).cpu().numpy(), rows['labels'])
    assert np.array_equal(torch.cat([t[2] for t in e0[1][1]]).cpu().numpy().view(np.int32), rows['masks'].view(np.int32))
    want = torch.from_numpy(ref.u8_table()[ref.augment_tiles_ref(bank.tiles, tab.cells, tab.crop, 64, 2, 96, 114)]).to(torch.bfloat16)
    assert torch.equal(e0[1][0].cpu().view(torch.int16), want.view(torch.int16))
    # masks=False on the same bank, and the bank without its map, take the two launches of the detection path: same boxes as augment_boxes
    wb, wl, wi, wc = ref.augment_boxes_ref(bank.boxes, bank.labels, bank.offsets, tab.cells, tab.crop, 64, 2, 96)
    plain_bank = augment.TileBank(bank.tiles, bank.boxes, bank.labels, bank.offsets)
    from metayolo.datasets import DeviceTiles
    for other in (masked_loader(masks=False)[0], DeviceTiles(plain_bank, hyp, 4, 2, rank=0, seed=0, device=DEV)):
        assert not other.masks
        batches = list(other)
        anns = [t['anns']['det'][0] for t in batches[1][1]]
        assert all('masks' not in a for a in anns)
        assert np.array_equal(torch.cat([a['boxes'] for a in anns]).cpu().numpy().view(np.int32), wb.view(np.int32))


def test_device_tiles_batch_with_masks_trains_the_mask_branch():
    from metayolo.models.yolo import Model
    loader, bank, hyp = masked_loader(steps=1)
    cfg = synth.make_cfg('n', 2)
    cfg['headers'][0][3][3] = 1                                  # the mask branch, as tests/test_gpu_mask.py builds it
    model = Model(cfg, synth.make_hyp())
    assert not model.load_state_dict(synth.mask_state_dict(model), strict=False).unexpected_keys
    model = model.to(DEV).train()
    imgs, targets = next(iter(loader))
    assert loader.d2h_copies == 1
    like = synth.synth_targets(4, 96, 2, nmin=2, nmax=3, seed=0, masks=True)
    for t, s in zip(targets, like):
        assert set(t) == set(s) and set(t['anns']['det'][0]) == set(s['anns']['det'][0])
        a = t['anns']['det'][0]
        assert a['masks'].shape == (len(a['boxes']), 28, 28) and a['masks'].dtype == like[0]['anns']['det'][0]['masks'].dtype
    assert sum(len(t['anns']['det'][0]['boxes']) for t in targets) > 0
    losses, _ = model(torch.stack(list(imgs)), targets, compute_masks=True)
    l = losses['det']
    assert torch.isfinite(l['det_loss']).all() and torch.isfinite(l['mask_loss']).all()
    (l['det_loss'] + l['mask_loss']).backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads)


def train_cmd(tmp_path, path, name):
    return [sys.executable, 'train.py', '--variant', 'n', '--nc', '2', '--batch-size', '8', '--imgsz', '128', '--epochs', '1', '--steps-per-epoch', '4',
            '--val-batches', '1', '--project', str(tmp_path), '--name', name, '--exist-ok', '--tile-bank', path, '--k-mosaic', '2', '--patch-size', '96',
            '--degrees', '10', '--perspective', '0.0005', '--masks']


def test_train_py_trains_masks_on_a_tile_bank(tmp_path):
    path = str(tmp_path / 'bank.npz')
    synth.synth_tile_bank(8, 128, 2, seed=3, instances=True).save(path)
    p = subprocess.run(train_cmd(tmp_path, path, 'bank'), cwd=ROOT, env=dict(os.environ, YOLOv5_VERBOSE='true'), capture_output=True, text=True,
                       timeout=500)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert 'epochs completed' in p.stdout + p.stderr and 'it 3/3' in p.stdout + p.stderr
    ck = torch.load(tmp_path / 'bank' / 'weights' / 'last.pt', map_location='cpu')
    assert all(torch.isfinite(v).all() for v in ck['model'].values() if v.dtype.is_floating_point)


def test_train_py_names_the_missing_instances_array(tmp_path):
    path = str(tmp_path / 'plain.npz')
    synth.synth_tile_bank(8, 128, 2, seed=3).save(path)
    p = subprocess.run(train_cmd(tmp_path, path, 'plain'), cwd=ROOT, env=dict(os.environ, YOLOv5_VERBOSE='true'), capture_output=True, text=True,
                       timeout=500)
    assert p.returncode != 0 and 'instances' in p.stdout + p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
