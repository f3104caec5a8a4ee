"""Synthetic tile stream with the reference loader's batch schema (reference: metayolo/datasets.py:462-519 target dict,
:850-870 create_dataloader, engines/torch_utils.py:172 collate).  BASELINE.json's workload is synthetic 640x640 RGB tiles;
the reference's CSV/cv2/albumentations pipeline is CPU image I/O and out of scope.  DeviceTiles trains from an 8-bit
tile bank with the augmentation on the device; BankTiles validates on one, in order and unaugmented."""
import torch

from hd_yolo_amd import synth


class SyntheticTiles:
    """Iterable of (imgs: tuple of (3,H,W) float tensors in 0..1, targets: tuple of target dicts).  Each rank draws from its
    own seed offset (what DistributedSampler gives the reference: disjoint shards)."""

    def __init__(self, batch_size, imgsz, nc, steps, rank=0, seed=0, task='det', nmin=50, nmax=400, device=None, masks=False):
        self.batch_size, self.imgsz, self.nc, self.steps = batch_size, imgsz, nc, steps
        self.rank, self.seed, self.task, self.nmin, self.nmax, self.device, self.masks = rank, seed, task, nmin, nmax, device, masks
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return self.steps

    def __iter__(self):
        for i in range(self.steps):
            s = self.seed + 1000003 * self.rank + 7919 * self.epoch + i
            x = synth.synth_images(self.batch_size, self.imgsz, seed=s)
            t = synth.synth_targets(self.batch_size, self.imgsz, self.nc, nmin=self.nmin, nmax=self.nmax, seed=s, task=self.task, masks=self.masks)
            if self.device is not None:
                x = x.to(self.device, non_blocking=True)
            yield tuple(x.unbind(0)), t


class DeviceTiles:
    """Training batches augmented on the device from an 8-bit tile bank (hd_yolo_amd.augment.TileBank): the reference's training branch
    (metayolo/datasets.py TorchDataset.__getitem__ with train_proc: HSV, random projective, flips, k x k mosaic, random crop, small-object
    filter, normalised boxes) as two launches per batch (csrc/augment.hip).  Iterable like SyntheticTiles; yields (imgs, targets): imgs a
    tuple of (3, S, S) views of one (B, 3, S, S) `dtype` tensor in 0..1, targets the per-image dicts of the reference's schema with device
    tensors (views of the batch's compact arrays).

    `hyp` carries the reference's keys (degrees translate scale shear perspective hsv_h hsv_s hsv_v fliplr flipud transpose cval k_mosaic
    patch_size img_size); a missing one raises KeyError.  `cval` is the border value as the reference hands it to cv2 on an 8-bit image
    (rounded half to even and clamped to 0..255).  keep_res > 0, color_aug other than 'hsv' and albumentations are refused.

    A bank with an instance map (TileBank.instances) and `masks=True` (the default) adds `'masks'`: (n_i, 28, 28) fp32 views, to every
    image's annotations, by three more launches per batch (csrc/augment_masks.hip: mask extents, the compaction with the masked objects'
    boxes taken from their warped masks, the 28 x 28 targets); per buffer set it holds an extents workspace of batch_size * k^2 *
    bank.max_per_tile * 32 bytes and `cap` x 28 x 28 floats, so pass `cap` (rows of a batch) when the default, every box of every cell, is
    too much.  `masks=False`, or a bank without a map, takes the two launches and gives their bits.  Mask formats other than the instance
    map (a bank with a `masks` attribute) are refused.

    The loader works on its own stream, one batch ahead: batch i + 1 is issued before batch i is handed out, and the per-image row counts —
    the only device-to-host copy, one per batch — are waited for through an event recorded a whole step earlier.  Two buffer sets
    alternate: a batch is valid until the next one is handed out.  Every (seed, rank, epoch, step) has its own numpy Generator, mixed as
    SyntheticTiles mixes them."""

    def __init__(self, bank, hyp, batch_size, steps, rank=0, seed=0, device='cuda', dtype=torch.bfloat16, task='det', cap=None, masks=True):
        from hd_yolo_amd import augment
        self.k, self.patch, self.imgsz, self.cval = augment.check_hyp(hyp)
        if getattr(bank, 'masks', None) is not None:
            raise ValueError("DeviceTiles: mask targets travel as the bank's uint16 instance map (TileBank.instances); other formats are not supported")
        self.masks = bool(masks) and getattr(bank, 'instances', None) is not None
        self.hyp, self.bank, self.batch_size, self.steps, self.rank, self.seed, self.task = dict(hyp), bank, batch_size, steps, rank, seed, task
        self.device, self.dtype = torch.device(device), dtype
        if self.device.type != 'cuda':
            raise ValueError('DeviceTiles augments on the GPU: there is no CPU path (use SyntheticTiles without one)')
        n_cells = batch_size * self.k * self.k
        if n_cells > augment.MAX_CELLS:
            raise ValueError(f'DeviceTiles: batch_size * k_mosaic^2 = {n_cells} cells in a batch (at most {augment.MAX_CELLS})')
        if bank.device != self.device:
            bank.to(self.device)
        self.epoch = 0
        self.d2h_copies = 0                    # device-to-host copies this loader made (one per batch: the row counts)
        self.cap = int(cap) if cap is not None else max(n_cells * max(bank.max_per_tile, 1), 1)
        self.stream = torch.cuda.Stream(device=self.device)
        nbytes = n_cells * augment.CELL_BYTES + batch_size * 8
        B, S, dev = batch_size, self.imgsz, self.device
        self.slots = []
        for _ in range(2):
            self.slots.append({
                'host': torch.empty(nbytes, dtype=torch.uint8).pin_memory(), 'table': torch.empty(nbytes, dtype=torch.uint8, device=dev),
                'imgs': torch.empty((B, 3, S, S), dtype=dtype, device=dev), 'boxes': torch.empty((self.cap, 4), dtype=torch.float32, device=dev),
                'labels': torch.empty((self.cap,), dtype=torch.int64, device=dev), 'img': torch.empty((self.cap,), dtype=torch.float32, device=dev),
                'counts': torch.empty((B + 1,), dtype=torch.int32, device=dev), 'counts_host': torch.empty((B + 1,), dtype=torch.int32).pin_memory(),
                'event': torch.cuda.Event()})
            if self.masks:
                from hd_yolo_amd import ops
                self.pitch = max(bank.max_per_tile, 1)
                self.slots[-1].update({
                    'ws': torch.empty(ops.augment_mask_workspace_bytes(n_cells, self.pitch), dtype=torch.uint8, device=dev),
                    'ref': torch.empty((self.cap, 2), dtype=torch.int32, device=dev), 'total': torch.empty((1,), dtype=torch.int32, device=dev),
                    'masks': torch.empty((self.cap, augment.MASK_SIDE, augment.MASK_SIDE), dtype=torch.float32, device=dev)})
        self._size = torch.tensor([S, S], dtype=torch.int64)
        self._ids = [torch.tensor([i], dtype=torch.int64) for i in range(B)]

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return self.steps

    def _issue(self, step, slot):
        """draw, pack, upload and launch batch `step` into `slot` on the loader's stream"""
        from hd_yolo_amd import augment, ops
        rng = augment.step_rng(self.seed, self.rank, self.epoch, step)
        pars = augment.draw_params(rng, self.hyp, self.batch_size, self.bank.n)
        augment.cell_tables(pars, (self.bank.H, self.bank.W), out=slot['host'].numpy())
        n_cells = self.batch_size * self.k * self.k
        self.stream.wait_stream(torch.cuda.current_stream(self.device))      # the consumer is done with this slot's previous batch
        with torch.cuda.stream(self.stream):
            slot['table'].copy_(slot['host'], non_blocking=True)
            cells = slot['table'][:n_cells * augment.CELL_BYTES].view(n_cells, augment.CELL_BYTES)
            crop = slot['table'][n_cells * augment.CELL_BYTES:].view(torch.int32).view(self.batch_size, 2)
            ops.augment_tiles(self.bank.d_tiles, cells, crop, slot['imgs'], self.patch, self.k, self.cval)
            bank, nb = self.bank, len(self.bank.boxes)
            if self.masks:
                ops.augment_mask_extents(bank.d_instances, bank.d_boxes, bank.d_has_mask, bank.d_offsets, nb, cells, crop, self.patch, self.k,
                                         self.imgsz, slot['ws'], self.pitch)
                ops.augment_boxes_masks(bank.d_boxes, bank.d_labels, bank.d_has_mask, bank.d_offsets, nb, cells, crop, self.patch, self.k,
                                        self.imgsz, slot['ws'], self.pitch, slot['boxes'], slot['labels'], slot['img'], slot['ref'],
                                        slot['counts'][:self.batch_size], slot['counts'][self.batch_size:], slot['total'])
                ops.augment_mask_targets(bank.d_instances, bank.d_has_mask, bank.d_offsets, nb, cells, crop, self.patch, self.k, self.imgsz,
                                         slot['ws'], self.pitch, slot['boxes'], slot['ref'], slot['total'], slot['masks'])
            else:
                ops.augment_boxes(bank.d_boxes, bank.d_labels, bank.d_offsets, nb, cells, crop, self.patch, self.k, self.imgsz, slot['boxes'],
                                  slot['labels'], slot['img'], slot['counts'][:self.batch_size], slot['counts'][self.batch_size:])
            slot['counts_host'].copy_(slot['counts'], non_blocking=True)
            self.d2h_copies += 1
            slot['event'].record(self.stream)

    def _hand_out(self, slot):
        slot['event'].synchronize()
        torch.cuda.current_stream(self.device).wait_event(slot['event'])
        counts = slot['counts_host'].tolist()
        if counts[-1]:
            raise RuntimeError(f'DeviceTiles: a batch kept {sum(counts[:-1])} boxes, more than the capacity of {self.cap} rows: raise `cap`')
        counts = counts[:-1]
        total = sum(counts)
        boxes, labels = slot['boxes'][:total].split(counts), slot['labels'][:total].split(counts)
        targets = tuple({'image_id': self._ids[i], 'size': self._size,
                         'anns': {self.task: [{'size': self._size, 'boxes': boxes[i], 'labels': labels[i]}]}} for i in range(self.batch_size))
        if self.masks:
            for t, m in zip(targets, slot['masks'][:total].split(counts)):
                t['anns'][self.task][0]['masks'] = m
        return tuple(slot['imgs'].unbind(0)), targets

    def __iter__(self):
        if self.steps <= 0:
            return
        self._issue(0, self.slots[0])
        for i in range(self.steps):
            if i + 1 < self.steps:
                self._issue(i + 1, self.slots[(i + 1) % 2])
            yield self._hand_out(self.slots[i % 2])


def bank_batches(n, batch_size):
    """[(first, count)] of tiles 0 .. n - 1 in batches of batch_size: ceil(n / batch_size) of them, the last one partial"""
    if batch_size < 1:
        raise ValueError(f'batch_size={batch_size}')
    return [(first, min(batch_size, n - first)) for first in range(0, n, batch_size)]


def bank_origins(n, H):
    """the bank as one slide of n * H rows: tile t starts at (x0, y0) = (0, t * H); int32 (n, 2)"""
    import numpy as np
    out = np.zeros((n, 2), np.int32)
    out[:, 1] = np.arange(n, dtype=np.int64) * H
    return out


def bank_name(bank):
    path = getattr(bank, 'path', None)
    return f'tile bank {path}' if path else f'tile bank ({bank.n} tiles of {bank.H} x {bank.W})'


def check_bank_stride(bank, stride):
    """A validation bank runs at its own tile size (there is no resize), so both tile sides must be multiples of the model's largest stride."""
    stride = int(stride)
    for side, name in ((bank.H, 'height'), (bank.W, 'width')):
        if side % stride:
            raise ValueError(f'{bank_name(bank)}: tile {name} {side} is not a multiple of the model\'s largest stride {stride} '
                             '(validation runs a bank at its own tile size)')


class BankTiles:
    """Validation batches from an 8-bit tile bank (hd_yolo_amd.augment.TileBank) at the bank's own tile size: tile 0 .. n - 1 in order,
    ceil(n / batch_size) batches with the last one partial, no augmentation, no resize, no filtering of small boxes, no shuffling
    (set_epoch is a no-op).  Iterable like SyntheticTiles: yields (imgs, targets), imgs a tuple of (3, H, W) float32 tensors equal to
    tile.permute(2, 0, 1).float() / 255 (the correctly rounded quotient that hdy_slide_tiles_u8 writes), targets the per-image dicts of the
    reference's schema with device tensors: 'boxes' (n_t, 4) fp32 xyxy in PIXELS (the reference validates with normalize_box=augment, i.e.
    off) and 'labels' (n_t,) int64, views of the uploaded bank.  A bank with an instance map and masks=True (the default) adds
    'instances', the tile's (H, W) 16-bit map as DeviceAPMeter.add_batch_masks takes it — the bank's bits, a view; masks=True on a bank
    without `instances` silently gives box-only targets.

    For the 8-bit forward (Model.forward_tiles) the loader is also the bank as one slide: `slide` = d_tiles viewed (n * H, W, C), `origins`
    the int32 device table of (0, t * H), `tile` = (H, W), built once, and u8_batches() yields ((first, count), targets) without making a
    float batch; val_nuclei.run takes that path when handed a BankTiles.  check_stride(stride) refuses tile sides that are no multiple of
    a model's largest stride (where the model is known: val_nuclei.run and the command lines)."""

    def __init__(self, bank, batch_size, device='cuda', task='det', masks=True):
        self.bank, self.batch_size, self.task = bank, int(batch_size), task
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if bank.device != self.device:
            bank.to(self.device)
        self.masks = bool(masks) and getattr(bank, 'instances', None) is not None
        n, H, W, C = bank.d_tiles.shape
        if not bank.d_tiles.is_contiguous():
            raise ValueError(f'{bank_name(bank)}: {C}-byte pixels with strides {tuple(bank.d_tiles.stride())}: the tiles must be contiguous to be '
                             f'read as one slide of {n * H} rows')
        self.batches = bank_batches(n, self.batch_size)
        self.tile = (H, W)
        self.slide = bank.d_tiles.view(n * H, W, C)
        self.origins = torch.from_numpy(bank_origins(n, H)).to(self.device)
        self._size = torch.tensor([H, W], dtype=torch.int64)
        self._offsets = [int(v) for v in bank.offsets]
        import numpy as np
        self._quotients = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255)).to(self.device)

    def set_epoch(self, epoch):
        pass

    def __len__(self):
        return len(self.batches)

    def check_stride(self, stride):
        check_bank_stride(self.bank, stride)

    def _targets(self, first, count):
        bank, o = self.bank, self._offsets
        out = []
        for t in range(first, first + count):
            ann = {'size': self._size, 'boxes': bank.d_boxes[o[t]:o[t + 1]], 'labels': bank.d_labels[o[t]:o[t + 1]]}
            if self.masks:
                ann['instances'] = bank.d_instances[t]
            out.append({'image_id': torch.tensor([t], dtype=torch.int64), 'size': self._size, 'anns': {self.task: [ann]}})
        return tuple(out)

    def u8_batches(self):
        """((first, count), targets) per batch: tiles [first, first + count) of `slide` / `origins`"""
        for first, count in self.batches:
            yield (first, count), self._targets(first, count)

    def __iter__(self):
        for first, count in self.batches:
            # byte / 255 through a table of the 256 correctly rounded quotients: a device division by a scalar multiplies by its reciprocal
            x = self._quotients[self.bank.d_tiles[first:first + count, :, :, :3].permute(0, 3, 1, 2).to(torch.int32)]
            yield tuple(x.unbind(0)), self._targets(first, count)
