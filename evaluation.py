#!/usr/bin/env python3
"""Inference caller on the MI355X path (reference: evaluation.py:27-66 build_model, :69-80 attempt_load_model,
:83-150 inference_on_loader_yolov5, and the whole-slide helpers Detect.merge_outputs / rescale_outputs, yolo_head.py:450-471).

    build_model(path | state | Model, ref_model=None, half=True, extra_configs={}) -> (model, deployed)
    attempt_load_model(path | [paths], ...)                                        -> single pair, or (Ensemble, Ensemble)
    inference_on_loader_yolov5(deployed, loader, device, input_size=640, compute_masks=False) -> (results, seconds per image)
    inference_on_slide(deployed, slide, tile=640, overlap=64, ...)                 -> one merged {'boxes','scores','labels'} per task
                       (slide on the GPU: float (3, H, W) in 0..1, or 8-bit (H, W, 3 | 4) as slide readers deliver it)

What differs from the reference, on purpose: `torch.jit.script(Deploy(model))` has no counterpart — the eval launch list of the
wrapped Model is the deployed artefact (yolo.Deploy) —, checkpoints may hold state_dicts instead of pickled modules
(engines/general.checkpoint_state reads both), and display / plotting / pandas evaluation tables are CPU-side reporting outside the
hot path.  Timing brackets exactly what the reference brackets (:98-105: resize + model call), with a device
synchronisation on both sides because HIP launches are asynchronous.

    python evaluation.py --variant s --nc 8 --imgsz 640 --batch-size 32 --batches 4 [--weights w.pt] [--slide 2048 [--u8] [--min-tissue 0.05] [--score] [--masks --label-map]]
    (--score with --masks --label-map also scores the synthetic sets as segmentations: score_slide_masks, mask mAP@.5, PQ / AJI / Dice)
"""
import argparse
import os
import sys
import time
from collections import OrderedDict

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')               # before the HIP runtime loads: see hd_yolo_amd/__init__.py
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault('YOLOv5_VERBOSE', 'false')

from metayolo.engines.general import checkpoint_state, intersect_dicts, manipulate_header_label_order  # noqa: E402
from metayolo.models.utils_general import nms, scale_coords  # noqa: E402
from metayolo.models.yolo import Deploy, Ensemble, Model  # noqa: E402
from val_nuclei import flatten_onehot_objects  # noqa: E402


@torch.no_grad()
def build_model(model_path, ref_model=None, half=True, extra_configs={}):
    """Checkpoint (path, loaded checkpoint or state_dict) -> (Model in eval mode, Deploy wrapper).  `ref_model` supplies cfg / hyp
    when the checkpoint is a bare state_dict (reference :30-36); EMA weights are preferred (:34); anchors come from the cfg (:37)."""
    ckpt = torch.load(model_path, map_location='cpu', weights_only=False) if isinstance(model_path, (str, os.PathLike)) else model_path
    if isinstance(ckpt, Model):
        ref_model, csd = ref_model or ckpt, ckpt.state_dict()
    else:
        holder = None
        if isinstance(ckpt, dict) and 'model' in ckpt:
            holder = ckpt['ema'] if ckpt.get('ema') is not None else ckpt['model']
        if isinstance(holder, torch.nn.Module):
            ref_model = ref_model or holder
        assert ref_model is not None, 'model cannot be None if only state_dict is given.'
        csd = checkpoint_state(ckpt, prefer_ema=True)
    csd = OrderedDict((k, v) for k, v in csd.items() if 'anchor' not in k)
    model = Model(ref_model.cfg, ref_model.hyp)
    model.load_state_dict(intersect_dicts(csd, model.state_dict()), strict=False)
    for key, cfgs in extra_configs.get('headers', {}).items():         # {'headers': {'det': {'label_map': [...], 'nms_params': {...}}}}
        if 'label_map' in cfgs:
            model.headers[key] = manipulate_header_label_order(model.headers[key], cfgs['label_map'])
        if 'nms_params' in cfgs:
            model.headers[key].nms_params = model.headers[key].get_nms_params(cfgs['nms_params'])
    model.eval()
    if half:
        model.half()
    return model, Deploy(model)


@torch.no_grad()
def attempt_load_model(weights_path, ref_model=None, half=True, extra_configs={}):
    if not isinstance(weights_path, (list, tuple)):
        return build_model(weights_path, ref_model=ref_model, half=half, extra_configs=extra_configs)
    pairs = [build_model(p, ref_model=ref_model, half=half, extra_configs=extra_configs) for p in weights_path]
    return Ensemble([m for m, _ in pairs]), Ensemble([d for _, d in pairs])


@torch.no_grad()
def inference_on_loader_yolov5(model, data_loader, device, input_size=640, compute_masks=False, **kwargs):
    """Timed loop of the reference (:83-150): stack, bilinear resize to `input_size`, model call, boxes back to the original frame with
    scale_coords(...).round(), multi-hot labels flattened, everything to the host.  Returns (list of per-image dicts, s / image)."""
    model.eval()
    model.to(device)
    results, total_time, n_images = [], 0.0, 0
    for images, _targets in data_loader:
        images = torch.stack(list(images)).to(device, non_blocking=True)
        ori_size = tuple(images.shape[-2:])
        torch.cuda.synchronize(device)
        st = time.time()
        size = (input_size, input_size) if isinstance(input_size, int) else tuple(input_size)
        inputs = images if size == ori_size else torch.nn.functional.interpolate(images.float(), size=size, mode='bilinear', align_corners=False)
        _, outputs = model(inputs, compute_masks=compute_masks)
        torch.cuda.synchronize(device)
        total_time += time.time() - st
        n_images += len(images)
        for output in outputs:
            for task_id in output:
                o = output[task_id]
                o['boxes'] = scale_coords(size, o['boxes'], ori_size).round()
                if o['labels'].dim() == 2:
                    o = flatten_onehot_objects(o)
                output[task_id] = {k: v.detach().cpu() for k, v in o.items()}
            results.append(output)
    return results, total_time / max(n_images, 1)


def slide_rois(height, width, tile, overlap):
    """Top-left corners (x0, y0) of `tile`-sized windows covering the slide with at least `overlap` pixels shared between neighbours;
    the last window of a row / column is shifted back inside the slide."""
    def starts(n):
        if n <= tile:
            return [0]
        step = tile - overlap
        s = list(range(0, n - tile, step)) + [n - tile]
        return sorted(set(s))
    return [(x0, y0) for y0 in starts(height) for x0 in starts(width)]


def slide_tile_table(height, width, tile, overlap, counts=None, min_tissue=0.0):
    """Host side of the device tile table of an 8-bit slide: int32 array (n, 2) of (x0, y0) in the order of slide_rois.  With per-tile
    tissue counts (ops.slide_tissue: pixels of the window that are not background) the rows with count < min_tissue * tile * tile are
    dropped.  The rule is this project's own: the reference has no blank-tile skipping."""
    import numpy as np
    table = np.asarray(slide_rois(height, width, tile, overlap), dtype=np.int32).reshape(-1, 2)
    if counts is not None and min_tissue > 0.0:
        counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        assert len(counts) == len(table), (len(counts), len(table))
        table = table[counts >= float(min_tissue) * tile * tile]
    return table


def _check_slide(slide):
    """what inference_on_slide accepts, said in one place (a clear error here instead of an assert deep inside a launch wrapper)"""
    if not isinstance(slide, torch.Tensor):
        raise TypeError(f'inference_on_slide: slide must be a torch tensor on the GPU, got {type(slide).__name__}')
    if not slide.is_cuda:
        raise ValueError('inference_on_slide: the slide must be on the GPU (slide.cuda()): a float (3, H, W) tensor in 0..1, or the 8-bit '
                         '(H, W, 3) RGB / (H, W, 4) RGBA tensor a slide reader delivers')
    if slide.dtype == torch.uint8:
        ok = slide.dim() == 3 and slide.shape[2] in (3, 4) and slide.stride(2) == 1 and slide.stride(1) == slide.shape[2] \
            and (slide.shape[0] <= 1 or slide.stride(0) >= slide.shape[1] * slide.shape[2]) and slide.numel() > 0
        if not ok:
            raise ValueError(f'inference_on_slide: an 8-bit slide must be (H, W, 3) RGB or (H, W, 4) RGBA with interleaved pixels and dense '
                             f'rows (stride(2) == 1, stride(1) == C, any row stride); got shape {tuple(slide.shape)}, strides '
                             f'{tuple(slide.stride())}.  A planar (3, H, W) uint8 tensor is not accepted: pass slide.permute(1, 2, 0).contiguous() '
                             f'or a float (3, H, W) tensor')
        return True
    if not slide.is_floating_point() or slide.dim() != 3:
        raise ValueError(f'inference_on_slide: a slide is a float (3, H, W) tensor in 0..1 or an 8-bit (H, W, 3 | 4) tensor, got {slide.dtype} '
                         f'{tuple(slide.shape)}')
    return False


@torch.no_grad()
def inference_on_slide(model, slide, tile=640, overlap=64, batch_size=32, scale=1.0, iou_thres=None, compute_masks=False, min_tissue=0.0,
                       background=220, label_map=False, measure=False, neighbors=None, outlines=False, graph=None, stain_normalize=None, info=None):
    """Whole-slide detection as the reference's ROI protocol composes it: tiles of one amplification are run in batches, each tile's
    detections carry their 'roi' offset, `Detect.merge_outputs` shifts and concatenates them (yolo_head.py:450-462), overlapping
    windows are de-duplicated by one class-agnostic NMS on the MI355X kernel (as Ensemble.merge does, yolo.py:189-199), and
    `Detect.rescale_outputs` maps the boxes to another amplification (:464-471).

    slide, on the GPU: (3, H, W) float in 0..1, or the slide as readers deliver it — uint8 (H, W, 3) RGB or (H, W, 4) RGBA (alpha ignored)
    with interleaved pixels and any row stride, so a crop of a larger slide is a view.  The 8-bit slide is never converted as a whole:
    tiles are gathered straight into the network's input buffer (pixel / 255, correctly rounded), and for single-label headers the
    detections stay on the device until the merge — one read of a device cursor per slide, none per batch; with compute_masks each batch's
    masks are made in compacted order beside the append (Detect.masks_device: one read of the batch's counts, which size the mask head's
    launches) and joined once at the end (HDY_DEVICE_MASKS=0: the per-tile Python merge).
    min_tissue > 0 (8-bit slides only; not in the reference): tiles with fewer than min_tissue * tile * tile pixels that are not
    background are skipped, a pixel being background when min(R, G, B) >= background.  0.0 keeps every tile and launches nothing.
    label_map=True (with compute_masks, on a model with a mask branch; not in the reference, which pastes per image: val_nuclei.py:169-176):
    every task with masks gains 'label_map', the int32 (round(H * scale), round(W * scale)) nucleus segmentation of the slide drawn from the
    final boxes and masks (-1 background, else the row of the returned detection that owns the pixel: slide_label_map), and 'areas'.
    measure=True (with label_map): every task with a label map gains 'nuclei', the table of slide_nucleus_table: position, size, axes,
    orientation, outline and border contact of every detection from one more pass over the map, and its mean / standard deviation per stain
    channel when the slide is 8-bit and scale == 1.0 (map and slide then share a grid; otherwise the table has no 'mean_rgb' / 'std_rgb')
    (not in the reference, which measures nothing).  measure=False launches nothing new.
    neighbors=(r1, r2, ...) (with measure; up to four increasing radii in pixels of the returned coordinates): 'nuclei' gains 'neighbors',
    'nearest_dist' and 'nearest_row', the columns of slide_neighborhood (hd_yolo_amd/spatial.py) for the header's classes.  None launches
    nothing new.
    outlines=True (with measure): 'nuclei' gains the shape columns of slide_nucleus_outlines (hd_yolo_amd/outline.py: outline vertices and
    edges, enclosed area, simple, convex area and perimeter, solidity, convexity, the Feret diameters) and the task gains 'polygons' =
    (offsets, verts), the outline of every nucleus as a polygon in the returned coordinates.  False launches nothing new.
    graph=(k, max_px) (with measure): the task gains 'graph', the cell graph of slide_cell_graph: every nucleus joined to its k <= 16 nearest
    nuclei of the header's classes within max_px pixels of the returned coordinates, with the union edge list.  'nuclei' keeps its columns.
    None launches nothing new.
    stain_normalize (8-bit slides only; not in the reference): True estimates the slide's stain vectors from every 4th pixel
    (hd_yolo_amd/stain.py: estimate_stains(slide, step=4), Macenko's method on integer device counts) and recolours the slide to the default
    StainTarget into a new slide before the tile gather; a StainEstimate is used as given.  Everything downstream, the measured stain
    columns included, sees the normalised slide.  `info`, a dict, receives the estimate as 'stain_estimate'.  None does not touch the path."""
    u8 = _check_slide(slide)
    if stain_normalize is not None and stain_normalize is not False:
        if not u8:
            raise ValueError('inference_on_slide: stain_normalize applies to 8-bit slides (the stain model is defined on 8-bit RGB values)')
        from hd_yolo_amd import stain as hstain
        estimate = hstain.estimate_stains(slide, step=4) if stain_normalize is True else stain_normalize
        slide = hstain.normalize_slide(slide, estimate)
        if info is not None:
            info['stain_estimate'] = estimate
    if measure and not label_map:
        raise ValueError('inference_on_slide: measure=True needs label_map=True (the nuclei are measured on the label map)')
    if neighbors is not None and not measure:
        raise ValueError('inference_on_slide: neighbors needs measure=True (the neighbourhoods are those of the nucleus table)')
    if outlines and not measure:
        raise ValueError('inference_on_slide: outlines=True needs measure=True (the outlines start from the extents of the nucleus table)')
    if graph is not None and not measure:
        raise ValueError('inference_on_slide: graph needs measure=True (the nodes of the graph are the rows of the nucleus table)')
    stained = slide if measure and u8 and float(scale) == 1.0 else None
    inner = model._model if isinstance(model, Deploy) else model
    if label_map:
        headers = getattr(inner, 'headers', None)
        if not compute_masks:
            raise ValueError('inference_on_slide: label_map=True needs compute_masks=True (the map is drawn from the masks)')
        if headers is None or not any(getattr(h, 'nc_masks', 0) > 0 for h in headers.values()):
            raise ValueError('inference_on_slide: label_map=True needs a model with a mask branch')
    if u8:
        return _inference_on_slide_u8(model, slide, tile, overlap, batch_size, scale, iou_thres, compute_masks, min_tissue, background, label_map,
                                      measure, stained, neighbors, outlines, graph)
    if min_tissue:
        raise ValueError('inference_on_slide: min_tissue applies to 8-bit slides (the background rule is defined on 8-bit RGB values)')
    _, H, W = slide.shape
    rois = slide_rois(H, W, tile, overlap)
    per_task = {}
    for i in range(0, len(rois), batch_size):
        chunk = rois[i:i + batch_size]
        x = slide.new_zeros((len(chunk), 3, tile, tile))
        for j, (x0, y0) in enumerate(chunk):
            patch = slide[:, y0:y0 + tile, x0:x0 + tile]
            x[j, :, :patch.shape[1], :patch.shape[2]] = patch
        _, outputs = model(x, compute_masks=compute_masks)
        for (x0, y0), out in zip(chunk, outputs):
            for task_id, o in out.items():
                per_task.setdefault(task_id, []).append(dict(o, roi=(float(x0), float(y0))))
    if label_map:
        _zero_row_masks(inner.headers, per_task)
    merged = {task_id: inner.headers[task_id].merge_outputs(parts) for task_id, parts in per_task.items()}
    return _finish_slide(inner, merged, H, W, overlap, scale, iou_thres, label_map, measure, stained, neighbors, outlines, graph)


def _zero_row_masks(headers, per_task):
    """label_map path: a tile without detections carries no 'masks' key and Detect.merge_outputs looks only at the first tile, so such tiles get
    a zero-row 'masks' before the merge (merge_outputs itself keeps the reference's text)"""
    for task_id, parts in per_task.items():
        h = headers[task_id]
        if getattr(h, 'nc_masks', 0) > 0:
            for i, o in enumerate(parts):
                if 'masks' not in o:
                    parts[i] = dict(o, masks=o['boxes'].new_zeros((0, 1, h.mask_output_size, h.mask_output_size), dtype=torch.float32))


@torch.no_grad()
def slide_label_map(result, size, window=None, threshold=0.5):
    """One task's result ({'boxes', 'masks', ...} as inference_on_slide(compute_masks=True) returns it, device tensors) -> (label_map, areas):
    the int32 map of the (H, W) = size canvas, or of its window (x0, y0, w, h) — -1 background, else the row of the detection that owns the
    pixel, the lowest row (= highest score after the slide NMS) among those whose pasted mask is >= threshold there — and the int32 pixel
    count of every row.  Two launches (ops.paste_label_map, ops.label_areas) for any number of detections; nothing is read back."""
    from hd_yolo_amd import ops
    if 'masks' not in result:
        raise ValueError("slide_label_map: the result has no 'masks' (run the model with compute_masks=True)")
    lm = ops.paste_label_map(result['masks'], result['boxes'], size, window=window, threshold=threshold)
    return lm, ops.label_areas(lm, len(result['boxes']))


@torch.no_grad()
def slide_nucleus_table(result, slide=None, window=None, threshold=0.5):
    """One task's result -> the nucleus table (hd_yolo_amd/measure.py: nucleus_table), a dict of device tensors with one row per detection:
    area, centroid, bbox, major / minor axis, eccentricity, orientation, equivalent diameter, perimeter and border edges, touches_border,
    compactness, labels, scores and, with the 8-bit `slide` the map was drawn on ((H, W, 3 | 4) uint8), mean_rgb / std_rgb.  The result's
    'label_map' is measured; a result without one ('boxes' and 'masks' only) gets it from slide_label_map at `threshold`.  window =
    (x0, y0, w, h): the part of the slide the map holds (default: all of it, from (0, 0)); positions in the table are slide coordinates.
    One measuring pass (ops.label_measure) whatever the number of detections, moments taken about each box's truncated corner; nothing is
    read back."""
    from hd_yolo_amd import measure as hmeasure
    from hd_yolo_amd import ops
    lm = result.get('label_map')
    if lm is None:
        if window is None and slide is None:
            raise ValueError("slide_nucleus_table: a result without 'label_map' needs the slide or a window to size the map")
        size = (int(slide.shape[0]), int(slide.shape[1])) if slide is not None else (int(window[1] + window[3]), int(window[0] + window[2]))
        lm, _ = slide_label_map(result, size, window=window, threshold=threshold)
    h, w = lm.shape
    x0, y0 = (0, 0) if window is None else (int(window[0]), int(window[1]))
    if window is not None and (int(window[2]), int(window[3])) != (w, h):
        raise ValueError(f'slide_nucleus_table: window {tuple(window)} does not match the {h} x {w} label map')
    boxes = result['boxes'].detach().to(lm.device).reshape(-1, 4).float()
    corner = torch.nan_to_num(boxes[:, :2], nan=0.0) - boxes.new_tensor([x0, y0])
    hi = boxes.new_tensor([w - 1, h - 1])
    origin = torch.minimum(corner.clamp(min=0), hi).to(torch.int32)              # truncated and clamped into the window
    sums, extent = ops.label_measure(lm, len(boxes), image=slide, window=(x0, y0), origin=origin)
    return hmeasure.nucleus_table(sums, extent, origin=origin, offset=(x0, y0), labels=result.get('labels'), scores=result.get('scores'),
                                  stain=slide is not None)


@torch.no_grad()
def slide_neighborhood(result, nc, radii_px, field_px=None):
    """One task's result -> its neighbourhood columns (hd_yolo_amd/spatial.py: neighborhood), device tensors: 'neighbors' int32 (N, K, nc), the
    other nuclei of every class within each of the K radii (pixels of the result's coordinates) of every nucleus; 'nearest_dist' float64
    (N, nc) / 'nearest_row' int32 (N, nc), the nearest nucleus of every class within the largest radius (NaN / -1 = none); with field_px,
    'density' int32 (gy, gx, nc), the nuclei of every class per field.  Positions are the centroids of the result's 'nuclei' table (rows that
    own no pixel are absent), or the box centres of a result without one; the class of a row is labels - 1.  With a 'label_map' in the result
    its size bounds the search grid and nothing is read back."""
    from hd_yolo_amd import spatial
    table = result.get('nuclei')
    if table is None:
        table = result
    lm = result.get('label_map')
    return spatial.neighborhood(table, nc, radii_px, field_px=field_px, size=None if lm is None else tuple(lm.shape))


def _map_and_extents(who, result, window):
    """(label map, nuclei table, R, extent, x0, y0) of one task's result: the int32 (R, 4) boxes of the table's 'bbox' in the map's own
    coordinates, as the label passes read them, and the origin of `window` = (x0, y0, w, h) on the slide (None: the map starts at (0, 0))"""
    lm, table = result.get('label_map'), result.get('nuclei')
    if lm is None or table is None:
        raise ValueError(f"{who}: the result needs 'label_map' and 'nuclei' (inference_on_slide(..., label_map=True, measure=True))")
    x0, y0 = (0, 0) if window is None else (int(window[0]), int(window[1]))
    n = table['area']
    shift = torch.tensor([x0, y0, x0, y0], dtype=torch.int64, device=lm.device)
    extent = torch.where((n > 0)[:, None], table['bbox'] - shift, table['bbox']).to(torch.int32)        # nucleus_table shifted the rows that own pixels
    return lm, table, len(n), extent, x0, y0


@torch.no_grad()
def slide_nucleus_outlines(result, window=None):
    """One task's result with its 'label_map' and 'nuclei' (slide_nucleus_table) -> (shape columns, (offsets, verts)): the columns of
    hd_yolo_amd/outline.py's shape_table (outline_vertices, outline_edges, enclosed_area, simple, convex_area, solidity, convex_perimeter,
    convexity, feret_max, feret_min, feret_ratio; device tensors, one row per detection) and the outline of every nucleus as a polygon,
    vertices of nucleus r = verts[offsets[r]:offsets[r + 1]] in the table's coordinates (slide pixels at the map's magnification).  The
    extents are the table's 'bbox': nothing is measured again.  window = (x0, y0, w, h): the part of the slide the map holds, as it was given
    to slide_nucleus_table.  Three passes (ops.label_outline: count and write; ops.label_hull); the number of vertices is read back once, to size verts."""
    from hd_yolo_amd import ops
    from hd_yolo_amd import outline as houtline
    lm, table, R, extent, x0, y0 = _map_and_extents('slide_nucleus_outlines', result, window)
    offsets, verts, counts = ops.label_outline(lm, R, extent)
    hull_i, hull_f = ops.label_hull(lm, R, extent)
    sums = torch.zeros((R, 7), dtype=torch.int64, device=lm.device)
    sums[:, 0], sums[:, 6] = table['area'], table['perimeter_edges']
    columns = houtline.shape_table(sums, counts, hull_i, hull_f)
    if x0 or y0:
        verts = verts + torch.tensor([x0, y0], dtype=torch.int32, device=lm.device)
    return columns, (offsets, verts)


@torch.no_grad()
def slide_nucleus_texture(result, slide, window=None, stain='hematoxylin', levels=16, matrix=None):
    """One task's result with its 'label_map' and 'nuclei' (slide_nucleus_table) and the 8-bit `slide` the map was drawn on ((H, W, 3 | 4)
    uint8) -> the texture columns of hd_yolo_amd/texture.py's texture_table, float64 device tensors with one row per detection: the
    statistics of the nucleus's levels of `stain` ('tex_level_mean', '_std', '_skewness', '_kurtosis', '_entropy', '_min', '_median', '_max'),
    the mean and the range over four directions of the 13 Haralick features of its co-occurrence matrices ('tex_contrast_mean',
    'tex_contrast_range', ...) and 'tex_flags'.  stain: 'hematoxylin', 'eosin', 'residual' (colour deconvolution), 'gray', 'r', 'g', 'b'; levels
    8, 16 or 32; matrix: the stain matrix of the deconvolution (None: Ruifrok-Johnston; hd_yolo_amd.stain.estimate_stains(slide).matrix: the
    slide's own).  The extents are the table's 'bbox': nothing is measured again.  window = (x0, y0, w, h): the part of the slide the map
    holds, as it was given to slide_nucleus_table.  One pass per 16 384 nuclei (ops.label_texture); nothing is read back."""
    from hd_yolo_amd import texture as htexture
    lm, _, R, extent, x0, y0 = _map_and_extents('slide_nucleus_texture', result, window)
    if slide is None or slide.dtype != torch.uint8:
        raise ValueError('slide_nucleus_texture: the texture is that of the 8-bit slide under the map ((H, W, 3 | 4) uint8)')
    return htexture.texture_table(lm, R, extent, slide, window=(x0, y0), stain=stain, levels=levels, matrix=matrix)


@torch.no_grad()
def slide_cell_graph(result, k, max_px, nc=None, mode='union'):
    """One task's result -> its cell graph (hd_yolo_amd/graph.py: knn_graph and edges), a dict of device tensors: 'knn_row' int32 (N, k), the
    rows of the k <= 16 nearest other nuclei within max_px pixels of the result's coordinates, nearest first, ties by the lowest row, -1
    padding; 'knn_dist' float64 (N, k) pixels (NaN padding); 'knn_count' int32 (N,); 'knn_mutual' bool (N, k); and the edge list of `mode`
    ('union', 'mutual' or 'directed'): 'edge_index' int64 (2, E), 'edge_dist' float64 (E,), 'edge_mutual' bool (E,).  Positions are those of
    slide_neighborhood: the centroids of the result's 'nuclei' table (rows that own no pixel are absent), or the box centres of a result
    without one.  With nc, the class of a row is labels - 1 and a row outside 0 .. nc - 1 is a query only; without it every present row is a
    node.  With a 'label_map' in the result its size bounds the search grid: the one scalar read back is the number of edges."""
    from hd_yolo_amd import graph as hgraph
    table = result.get('nuclei')
    if table is None:
        table = result
    lm = result.get('label_map')
    g = hgraph.knn_graph(table, k, max_px, nc=nc, size=None if lm is None else tuple(lm.shape))
    g.update(hgraph.edges(g, mode))
    return g


def save_cell_graph(path, graph, xy=None, labels=None):
    """the dict of slide_cell_graph as .npz (hd_yolo_amd/graph.py: one device-to-host copy); xy (N, 2) and labels (N,) go in beside it"""
    from hd_yolo_amd import graph as hgraph
    hgraph.save_cell_graph(path, graph, graph, xy=xy, labels=labels)


def save_polygons(path, polygons, scale=1.0, labels=None, scores=None):
    """the polygons of slide_nucleus_outlines as .npz or .geojson, by the extension of `path` (hd_yolo_amd/outline.py); scale: the
    magnification of the run, so that the file speaks the coordinates of the slide as it was given"""
    from hd_yolo_amd import outline as houtline
    houtline.save_polygons(path, polygons[0], polygons[1], scale=scale, labels=labels, scores=scores)


def save_nucleus_table(path, table):
    """a nucleus table as .npz or .csv, by the extension of `path` (hd_yolo_amd/measure.py: one device-to-host copy)"""
    from hd_yolo_amd import measure as hmeasure
    hmeasure.save_nucleus_table(path, table)


def _finish_slide(inner, merged, H, W, overlap, scale, iou_thres, label_map=False, measure=False, stained=None, neighbors=None,
                  outlines=False, graph=None):
    """everything after the merge: de-duplication of overlapping windows, clamp to the slide, rescale"""
    out = {}
    for task_id, r in merged.items():
        header = inner.headers[task_id]
        thr = header.nms_params['iou_thres'] if iou_thres is None else iou_thres
        if len(r['boxes']) and overlap > 0:
            keep = nms(r['boxes'], r['scores'], thr)
            r = {k: v[keep] for k, v in r.items()}
        r['boxes'][:, [0, 2]] = r['boxes'][:, [0, 2]].clamp(0, W)
        r['boxes'][:, [1, 3]] = r['boxes'][:, [1, 3]].clamp(0, H)
        out[task_id] = header.rescale_outputs(r, scale)
        if label_map and 'masks' in out[task_id]:
            size = (int(round(H * scale)), int(round(W * scale)))
            out[task_id]['label_map'], out[task_id]['areas'] = slide_label_map(out[task_id], size)
            if measure:
                out[task_id]['nuclei'] = slide_nucleus_table(out[task_id], slide=stained)
                if neighbors is not None:
                    columns = slide_neighborhood(out[task_id], header.nc, neighbors)
                    out[task_id]['nuclei'].update({k: columns[k] for k in ('neighbors', 'nearest_dist', 'nearest_row')})
                if outlines:
                    columns, out[task_id]['polygons'] = slide_nucleus_outlines(out[task_id])
                    out[task_id]['nuclei'].update(columns)
                if graph is not None:
                    out[task_id]['graph'] = slide_cell_graph(out[task_id], graph[0], graph[1], nc=header.nc)
    return out


def _inference_on_slide_u8(model, slide, tile, overlap, batch_size, scale, iou_thres, compute_masks, min_tissue, background, label_map=False,
                           measure=False, stained=None, neighbors=None, outlines=False, graph=None):
    from hd_yolo_amd import ops
    if isinstance(model, Ensemble):
        raise NotImplementedError('inference_on_slide: 8-bit slides run on one model (Model / Deploy); an Ensemble takes the float slide')
    inner = model._model if isinstance(model, Deploy) else model
    H, W, _ = slide.shape
    dev = slide.device
    table = slide_tile_table(H, W, tile, overlap)
    origins = ops.slide_origins(table, dev)                              # one upload per slide
    if min_tissue > 0.0:
        counts = ops.slide_tissue(slide, origins, tile, tile, background).cpu().numpy()      # one read, before the first batch
        table = slide_tile_table(H, W, tile, overlap, counts, min_tissue)
        origins = ops.slide_origins(table, dev) if len(table) else None
    n = len(table)
    headers = inner.headers
    want_masks = bool(compute_masks) and any(getattr(h, 'nc_masks', 0) > 0 for h in headers.values())
    # masks travel beside the append (Detect.masks_device, one compact tensor per batch); HDY_DEVICE_MASKS=0, several headers (the plan's mask
    # branch belongs to an only header) or a slide without tiles keep the Python merge
    dev_masks = want_masks and len(headers) == 1 and n > 0 and all(h.device_masks_on() for h in headers.values())
    on_device = not any(h.multi_label for h in headers.values()) and (not want_masks or dev_masks)
    if on_device:
        # slide-wide arrays per task, tiles x max_det rows (an exact upper bound), and a device cursor: every batch appends behind it
        acc, mask_parts = {}, {}
        for task_id, h in headers.items():
            cap = max(n, 1) * int(h.nms_params['max_det'])
            acc[task_id] = (torch.empty((cap, 4), dtype=torch.float32, device=dev), torch.empty((cap,), dtype=torch.float32, device=dev),
                            torch.empty((cap,), dtype=torch.int64, device=dev), torch.zeros((2,), dtype=torch.int32, device=dev))
        for i in range(0, n, batch_size):
            count = min(batch_size, n - i)                               # the last, smaller chunk runs at its own size
            _, outputs = model.forward_tiles(slide, origins, i, count, (tile, tile), compute_masks=dev_masks, device_outputs=True)
            for task_id, (boxes, scores, labels, n_keep, masks) in outputs.items():
                ops.slide_append(boxes, scores, labels, n_keep, origins, i, *acc[task_id])
                if masks is not None:                                    # the batch's compact masks, in the order the append wrote its rows
                    mask_parts.setdefault(task_id, []).append(masks)
        merged = {}
        for task_id, (boxes, scores, labels, cursor) in acc.items():
            rows, overflow = cursor.tolist()                             # the one device-to-host read of the slide (per task)
            if overflow:
                raise RuntimeError(f'inference_on_slide: the detections of task {task_id!r} passed the capacity of {len(scores)} rows')
            merged[task_id] = {'boxes': boxes[:rows], 'labels': labels[:rows], 'scores': scores[:rows]}
            if dev_masks:
                parts = mask_parts.get(task_id, [])
                made = sum(len(m) for m in parts)
                if made != rows:
                    raise RuntimeError(f'inference_on_slide: task {task_id!r} has {rows} detections and {made} masks')
                # keys as the Python merge leaves them on a slide without detections: zero-row masks with label_map (_zero_row_masks), none without
                # (Detect.merge_outputs looks at the first tile); storage is what the batches produced, joined once
                if parts:
                    merged[task_id]['masks'] = torch.cat(parts)
                elif label_map:
                    M = headers[task_id].mask_output_size
                    merged[task_id]['masks'] = boxes.new_zeros((0, 1, M, M), dtype=torch.float32)
    else:
        # multi-label rows and masks keep the Python merge; their tiles still come from the 8-bit slide
        per_task = {}
        for i in range(0, n, batch_size):
            count = min(batch_size, n - i)
            _, outputs = model.forward_tiles(slide, origins, i, count, (tile, tile), compute_masks=compute_masks)
            for (x0, y0), out in zip(table[i:i + count].tolist(), outputs):
                for task_id, o in out.items():
                    per_task.setdefault(task_id, []).append(dict(o, roi=(float(x0), float(y0))))
        if label_map:
            _zero_row_masks(headers, per_task)
        merged = {task_id: headers[task_id].merge_outputs(parts) for task_id, parts in per_task.items()}
    return _finish_slide(inner, merged, H, W, overlap, scale, iou_thres, label_map, measure, stained, neighbors, outlines, graph)


SCORE_CELL_SIDES = 4.0          # score_slide: side of an ordering cell, in mean box sides (a block of 256 rows then spans a few cells)


def _cell_order(boxes, x0, y0, cell, nx):
    """rows in row-major order of the cells their centres fall into (ties: lower row), by one torch.sort on the device"""
    cx = ((boxes[:, 0] + boxes[:, 2]) * 0.5 - x0).div(cell).floor().nan_to_num(0.0, 0.0, 0.0).clamp(0, nx - 1).to(torch.int64)
    cy = ((boxes[:, 1] + boxes[:, 3]) * 0.5 - y0).div(cell).floor().nan_to_num(0.0, 0.0, 0.0).clamp(0, nx - 1).to(torch.int64)
    return torch.sort(cy * nx + cx, stable=True)[1]


def slide_orders(pred_boxes, true_boxes):
    """the two permutations score_slide applies: both sets in the row-major order of the same coarse cells"""
    both = torch.cat([pred_boxes, true_boxes])
    finite = both[torch.isfinite(both).all(1)]
    if not len(finite):
        return torch.arange(len(pred_boxes), device=both.device), torch.arange(len(true_boxes), device=both.device)
    x0, y0 = finite[:, 0].min(), finite[:, 1].min()
    extent = torch.maximum(finite[:, 2].max() - x0, finite[:, 3].max() - y0).clamp_min(1e-6)
    mean_side = ((finite[:, 2] - finite[:, 0]).abs().mean() + (finite[:, 3] - finite[:, 1]).abs().mean()) * 0.5
    cell = torch.maximum(mean_side * SCORE_CELL_SIDES, extent / 4096.0)         # at most 4096 x 4096 cells
    return _cell_order(pred_boxes, x0, y0, cell, 4096), _cell_order(true_boxes, x0, y0, cell, 4096)


def _score_inputs(who, result, truth, iouv):
    """what both slide scorers start from: (iouv, or the ten thresholds 0.5 .. 0.95; fp32 scores; prediction labels; truth labels on the scores'
    device), flat; multi-label sets are refused"""
    if result['labels'].dim() != 1 or truth['labels'].dim() != 1:
        raise ValueError(f'{who}: multi-label results must be flattened first (val_nuclei.flatten_onehot_objects)')
    ps = result['scores'].detach().float().reshape(-1)
    return torch.linspace(0.5, 0.95, 10) if iouv is None else iouv, ps, result['labels'].detach(), truth['labels'].detach().to(ps.device)


@torch.no_grad()
def score_slide(result, truth, iouv=None, ignore=(-100, -1), info=None):
    """Scores one task's whole-slide result ({'boxes', 'scores', 'labels'}, as inference_on_slide returns it) against the slide's annotations
    ({'boxes', 'labels'}), all device tensors, as ONE image of 10^5-10^6 rows: the matching of APMeter without a dense IoU matrix
    (ops.ap_match).  Both sets are put in the row-major order of coarse cells (a few box sides wide) by a device sort, so that a block of
    predictions meets only the truth chunks around it; the original rows travel as pred_row / true_row, so ties resolve as in the given
    order, and the results are un-permuted.  Returns APMeter.ap_per_class's stats dict plus 'match' (int32 per detection: the row of its
    truth, or -1), 'match_iou' (fp32), 'hit' (threshold bits) and 'live', device tensors in the given order.  `info` receives chunks_visited / chunks_total / workspace_bytes."""
    from hd_yolo_amd import ops
    iouv, ps, pl, tl = _score_inputs('score_slide', result, truth, iouv)
    pb, tb = result['boxes'].detach().float().reshape(-1, 4), truth['boxes'].detach().float().reshape(-1, 4).to(ps.device)
    dev, n, m = pb.device, len(pb), len(tb)
    op, ot = slide_orders(pb, tb)
    off = lambda k: torch.tensor([0, k], dtype=torch.int32, device=dev)   # noqa: E731
    hit, live, match, miou = ops.ap_match(pb[op], ps[op], pl[op], off(n), tb[ot], tl[ot], off(m), iouv, ignore=ignore,
                                          pred_row=op.to(torch.int32), true_row=ot.to(torch.int32), info=info)
    inv = torch.empty_like(op)
    inv[op] = torch.arange(n, device=dev)
    hit, live, match, miou = hit[inv], live[inv], match[inv], miou[inv]
    match = torch.where(match >= 0, ot[match.clamp_min(0).to(torch.int64)].to(torch.int32), match) if m else match
    return _slide_stats(hit, live, match, miou, ps, pl, tl, iouv, ignore)


def _slide_stats(hit, live, match, miou, ps, pl, tl, iouv, ignore, **more):
    """APMeter.ap_per_class's stats dict from the device's per-detection hit bits and live flags (one copy of each compact array), plus the
    per-detection device tensors themselves and whatever `more` the caller adds"""
    from metayolo.models.metrics import ap_curves
    import numpy as np
    thr = np.asarray(iouv.tolist() if hasattr(iouv, 'tolist') else list(iouv), dtype=np.float32)
    bits, keep = hit.cpu().numpy().view(np.uint16), live.cpu().numpy().astype(bool)
    flags = ((bits[:, None] >> np.arange(len(thr), dtype=np.uint16)[None]) & 1).astype(bool)
    stats = ap_curves(flags[keep], ps.cpu().numpy()[keep], pl.cpu().numpy().astype(np.int64)[keep], tl.cpu().numpy().astype(np.int64), thr,
                      [int(v) for v in (ignore or ())])
    stats.update(match=match, match_iou=miou, hit=hit, live=live, **more)
    return stats


@torch.no_grad()
def slide_segmentation_summary(stats, pred_labels, true_labels, nc=None):
    """PQ / SQ / DQ / mPQ / AJI / Dice and the counts behind them (metayolo.models.metrics.segmentation_counts) from score_slide_masks'
    'pairs', 'pred_area' and 'true_area'; one device-to-host copy (and, with nc=None, one read of the largest label)"""
    from metayolo.models.metrics import segmentation_counts, segmentation_counts_to_host, segmentation_ratios
    c = segmentation_counts_to_host(segmentation_counts(stats['pairs'], stats['pred_area'], stats['true_area'], pred_labels, true_labels, nc=nc))
    return {**segmentation_ratios(c), **c}


@torch.no_grad()
def score_slide_masks(result, truth, iouv=None, ignore=(-100, -1), summaries=False):
    """Scores one task's whole-slide segmentation on mask IoU: `result` as inference_on_slide(..., compute_masks=True, label_map=True) returns it
    ({'label_map' int32 (H, W) with -1 background and else the owning row, 'scores', 'labels'}) against the slide's annotation
    ({'label_map' int32 (H, W) with negative background and else the object's row, 'labels'}), all device tensors.  Both sides are disjoint, so
    the mask IoU of every overlapping pair comes from one streaming pass over the two maps (ops.label_overlap: no dense (n_true, n_pred, H * W)
    product as in the reference's get_mask_ious) and the matching of APMeter from one more call (ops.mask_ap_match).  Returns score_slide's
    stats dict ('match' is the row of the matched object or -1) plus 'pred_area', 'true_area' (int32 pixels per row) and 'pairs' ((n, 3) int64:
    detection, object, shared pixels), device tensors.  summaries=True adds 'pq', 'sq', 'dq', 'mpq', 'aji', 'dice' and their counts
    (slide_segmentation_summary), formed from those.  One device-to-host read before the curves (the overlap status)."""
    from hd_yolo_amd import ops
    iouv, ps, pl, tl = _score_inputs('score_slide_masks', result, truth, iouv)
    if 'label_map' not in result or 'label_map' not in truth:
        raise ValueError("score_slide_masks: both sides need a 'label_map' (inference_on_slide(..., compute_masks=True, label_map=True))")
    pairs, pa, ta = ops.label_overlap(result['label_map'], truth['label_map'].to(ps.device), len(ps), len(tl))
    hit, live, match, miou = ops.mask_ap_match(pairs, pa, ta, ps, pl, tl, iouv, ignore=ignore)
    stats = _slide_stats(hit, live, match, miou, ps, pl, tl, iouv, ignore, pred_area=pa, true_area=ta, pairs=pairs)
    if summaries:
        stats.update(slide_segmentation_summary(stats, pl, tl))
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--weights', nargs='*', default=[], help='checkpoint(s); several = Ensemble; none = synthetic weights')
    ap.add_argument('--variant', default='s')
    ap.add_argument('--nc', type=int, default=8)
    ap.add_argument('--imgsz', type=int, default=640, help='network input size')
    ap.add_argument('--tile', type=int, default=0, help='original tile size (resized to --imgsz); default = --imgsz')
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--slide', type=int, default=0, help='also run one synthetic SxS slide through inference_on_slide')
    ap.add_argument('--u8', action='store_true', help='--slide: the synthetic slide as an 8-bit (H, W, 3) tensor (from the same seed), the way a slide reader delivers it')
    ap.add_argument('--min-tissue', type=float, default=0.0, help='--slide --u8: skip tiles with less than this fraction of non-background pixels')
    ap.add_argument('--score', action='store_true', help='--slide: also score a synthetic set of slide detections against a synthetic truth (score_slide)')
    ap.add_argument('--masks', action='store_true', help='--slide: also run the slide through a synthetic mask model (the tiny variant, one mask class, fp32) with compute_masks')
    ap.add_argument('--label-map', action='store_true', help='--slide --masks: paste the masks into one int32 label map of the slide (slide_label_map) and count the owned pixels')
    ap.add_argument('--measure', action='store_true', help='--slide --masks --label-map: measure every nucleus on the label map (slide_nucleus_table; stain columns with --u8)')
    ap.add_argument('--neighbors', default='', help='--measure: comma-separated radii in pixels, e.g. 32,64: neighbours of every class within each radius of every nucleus (slide_neighborhood)')
    ap.add_argument('--density', type=float, default=0.0, help='--neighbors: also count the nuclei of every class per field of this many pixels')
    ap.add_argument('--table', default='', help='--measure: write the nucleus table to this .npz or .csv file (save_nucleus_table)')
    ap.add_argument('--outlines', action='store_true', help='--measure: outline every nucleus as a polygon and add the hull descriptors: solidity, convexity, Feret diameters (slide_nucleus_outlines)')
    ap.add_argument('--polygons', default='', help='--outlines: write the polygons to this .geojson or .npz file (save_polygons)')
    ap.add_argument('--graph', default='', help='--measure: K,PX, e.g. 8,64: join every nucleus to its K <= 16 nearest nuclei within PX pixels (slide_cell_graph)')
    ap.add_argument('--texture', nargs='?', const='hematoxylin', default='', metavar='STAIN', help='--measure --u8: chromatin texture of every nucleus on this stain (hematoxylin, eosin, residual, gray, r, g, b): level statistics and Haralick features as tex_* columns of the table (slide_nucleus_texture)')
    ap.add_argument('--stain-normalize', action='store_true', help='--slide --u8: estimate the stain vectors of the slide (hd_yolo_amd/stain.py, Macenko on every 4th pixel), print them, and run the slide normalised to the default target (inference_on_slide(stain_normalize=...))')
    ap.add_argument('--stain-estimate', action='store_true', help='--slide --u8: estimate and print the stain vectors only; with --texture the tex_* columns are measured with the slide\'s own stain matrix')
    ap.add_argument('--graph-file', default='', help='--graph: write the cell graph to this .npz file (save_cell_graph)')
    ap.add_argument('--no-half', action='store_true')
    ap.add_argument('--device', default='')
    opt = ap.parse_args()
    from hd_yolo_amd import synth
    from metayolo.datasets import SyntheticTiles
    from metayolo.engines.torch_utils import select_device
    device = select_device(opt.device)
    ref = Model(synth.make_cfg(opt.variant, opt.nc), synth.make_hyp())
    if opt.weights:
        w = opt.weights if len(opt.weights) > 1 else opt.weights[0]
        model, deployed = attempt_load_model(w, ref_model=ref, half=not opt.no_half)
    else:
        ref.load_state_dict(synth.synth_state_dict(synth.shapes_of(ref), seed=0), strict=False)
        model, deployed = build_model(ref, half=not opt.no_half)
    loader = SyntheticTiles(opt.batch_size, opt.tile or opt.imgsz, opt.nc, opt.batches, seed=2024)
    inference_on_loader_yolov5(deployed, SyntheticTiles(opt.batch_size, opt.tile or opt.imgsz, opt.nc, 1, seed=1), device, input_size=opt.imgsz)   # warm-up: plans
    results, spi = inference_on_loader_yolov5(deployed, loader, device, input_size=opt.imgsz)
    n = sum(len(next(iter(r.values()))['boxes']) for r in results)
    print(f'{len(results)} tiles, {n} detections, {spi * 1e3:.3f} ms / tile ({1.0 / spi:.0f} tiles/s incl. host transfer of the results)')
    if opt.slide:
        slide = synth.synth_images(1, opt.slide, seed=5)[0].to(device)
        if opt.u8:
            slide = (slide * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
        est = None
        if opt.stain_normalize or opt.stain_estimate:
            if not opt.u8:
                ap.error('--stain-normalize and --stain-estimate need --u8')
            from hd_yolo_amd import stain as hstain
            from hd_yolo_amd import texture as htexture
            hstain.estimate_stains(slide, step=4)                             # warm-up
            torch.cuda.synchronize()
            t0 = time.time()
            est = hstain.estimate_stains(slide, step=4)
            torch.cuda.synchronize()
            dte = (time.time() - t0) * 1e3
            vec = lambda v: '(' + ', '.join(f'{float(c):.4f}' for c in v) + ')'      # noqa: E731
            off = [hstain.angle_between(est.matrix[i], htexture.stain_matrix()[i]) for i in range(2)]
            print(f'stain {opt.slide}x{opt.slide}: n_tissue {est.n_tissue} ({est.n_skipped} skipped, flags {est.flags}), haematoxylin {vec(est.matrix[0])} '
                  f'{off[0]:.2f} deg from Ruifrok, eosin {vec(est.matrix[1])} {off[1]:.2f} deg from Ruifrok, max_conc {vec(est.max_conc)} in {dte:.1f} ms')
        normalize = est if opt.stain_normalize else None
        torch.cuda.synchronize()
        t0 = time.time()
        out = inference_on_slide(deployed.to(device), slide, tile=opt.imgsz, batch_size=opt.batch_size, min_tissue=opt.min_tissue, stain_normalize=normalize)
        torch.cuda.synchronize()
        print(f'slide {opt.slide}x{opt.slide}: ' + ', '.join(f'{k}: {len(v["boxes"])} detections' for k, v in out.items()) + f' in {(time.time() - t0) * 1e3:.1f} ms')
        if opt.label_map and not opt.masks:
            ap.error('--label-map needs --masks')
        if opt.measure and not opt.label_map:
            ap.error('--measure needs --label-map')
        radii = tuple(float(r) for r in opt.neighbors.split(',')) if opt.neighbors else None
        if radii and not opt.measure:
            ap.error('--neighbors needs --measure')
        if opt.density and not radii:
            ap.error('--density needs --neighbors')
        if opt.outlines and not opt.measure:
            ap.error('--outlines needs --measure')
        if opt.polygons and not opt.outlines:
            ap.error('--polygons needs --outlines')
        knn = None
        if opt.graph:
            parts = opt.graph.split(',')
            if len(parts) != 2:
                ap.error('--graph takes K,PX, e.g. 8,64')
            knn = (int(parts[0]), float(parts[1]))
        if knn and not opt.measure:
            ap.error('--graph needs --measure')
        if opt.graph_file and not knn:
            ap.error('--graph-file needs --graph')
        if opt.texture and not (opt.measure and opt.u8):
            ap.error('--texture needs --measure and --u8')
        if opt.masks:
            cfg = synth.make_cfg('n', 2)
            cfg['headers'][0][3][3] = 1                                   # one mask class: the mask model of tests/test_gpu_mask.py
            mm = Model(cfg, synth.make_hyp(conf_thres=0.05))
            mm.load_state_dict(synth.mask_state_dict(mm), strict=False)
            mdep = Deploy(mm.to(device).eval())
            kw = dict(tile=min(opt.imgsz, opt.slide), batch_size=opt.batch_size, compute_masks=True, label_map=opt.label_map, measure=opt.measure,
                      neighbors=radii, outlines=opt.outlines, graph=knn, stain_normalize=normalize)
            inference_on_slide(mdep, slide, **kw)                         # warm-up: plans
            torch.cuda.synchronize()
            t0 = time.time()
            out = inference_on_slide(mdep, slide, **kw)
            torch.cuda.synchronize()
            dt = (time.time() - t0) * 1e3
            for k, v in out.items():
                line = f'masks {opt.slide}x{opt.slide}, task {k}: {len(v["boxes"])} detections'
                if 'areas' in v:
                    line += f', {int(v["areas"].sum())} owned pixels of {v["label_map"].numel()} ({int((v["areas"] > 0).sum())} detections own some)'
                print(line + f' in {dt:.1f} ms')
                if 'nuclei' in v:
                    torch.cuda.synchronize()
                    t0 = time.time()
                    nt = slide_nucleus_table(v, slide=slide if opt.u8 else None)
                    torch.cuda.synchronize()
                    dtm = (time.time() - t0) * 1e3
                    own = nt['area'] > 0
                    med = lambda c: float(c[own].median()) if bool(own.any()) else float('nan')
                    print(f'nuclei {opt.slide}x{opt.slide}, task {k}: {int(own.sum())} measured, {int((nt["touches_border"] & own).sum())} on the border, median '
                          f'area {med(nt["area"].double()):.1f} px, median major axis {med(nt["major_axis"]):.2f} px'
                          + (f', mean RGB {[round(float(c), 1) for c in nt["mean_rgb"][own].mean(0)]}' if 'mean_rgb' in nt and bool(own.any()) else '')
                          + f' in {dtm:.2f} ms')
                    if radii:
                        from hd_yolo_amd import spatial
                        nc_task = mdep._model.headers[k].nc
                        torch.cuda.synchronize()
                        t0 = time.time()
                        nb = slide_neighborhood(v, nc_task, radii, field_px=opt.density or None)
                        torch.cuda.synchronize()
                        dtn = (time.time() - t0) * 1e3
                        cls = v['labels'].to(torch.int64) - 1
                        pairs = spatial.interaction_matrix(nb['neighbors'], cls, nc_task)[-1].double()
                        per_class = torch.bincount(cls[own & (cls >= 0) & (cls < nc_task)], minlength=nc_task).double()
                        mean = (pairs / per_class[:, None]).tolist()
                        print(f'neighbours {opt.slide}x{opt.slide}, task {k}: {int(own.sum())} nuclei queried, mean neighbours within {radii[-1]:g} px per class '
                              f'pair (row: class of the nucleus, column: class of the neighbour) {[[round(x, 3) for x in r] for r in mean]}'
                              + (f', density grid {tuple(nb["density"].shape)} holds {int(nb["density"].sum())}' if 'density' in nb else '')
                              + f' in {dtn:.2f} ms')
                    if opt.outlines:
                        torch.cuda.synchronize()
                        t0 = time.time()
                        sh, polygons = slide_nucleus_outlines(v)
                        torch.cuda.synchronize()
                        dto = (time.time() - t0) * 1e3
                        done = sh['outline_vertices'] > 0
                        meds = lambda c: float(c[done].median()) if bool(done.any()) else float('nan')
                        print(f'outlines {opt.slide}x{opt.slide}, task {k}: {int(done.sum())} nuclei outlined with {len(polygons[1])} vertices, '
                              f'{float((sh["simple"] & done).sum()) / max(int(done.sum()), 1):.3f} simple, median solidity {meds(sh["solidity"]):.3f}, median '
                              f'Feret max / min {meds(sh["feret_max"]):.2f} / {meds(sh["feret_min"]):.2f} px in {dto:.2f} ms')
                        if opt.polygons:
                            save_polygons(opt.polygons, polygons, labels=v.get('labels'), scores=v.get('scores'))
                            print(f'polygons written to {opt.polygons}')
                    if knn:
                        torch.cuda.synchronize()
                        t0 = time.time()
                        cg = slide_cell_graph(v, knn[0], knn[1], nc=mdep._model.headers[k].nc)
                        torch.cuda.synchronize()
                        dtg = (time.time() - t0) * 1e3
                        E = cg['edge_index'].shape[1]
                        held = cg['knn_dist'][~torch.isnan(cg['knn_dist'])]
                        print(f'graph {opt.slide}x{opt.slide}, task {k}: {int((cg["knn_count"] > 0).sum())} nodes with neighbours of {len(cg["knn_count"])} '
                              f'rows, {E} edges (k = {knn[0]} within {knn[1]:g} px), {float(cg["edge_mutual"].sum()) / max(E, 1):.3f} mutual, median kNN '
                              f'distance {float(held.median()) if held.numel() else float("nan"):.2f} px in {dtg:.2f} ms')
                        if opt.graph_file:
                            xy = torch.stack([v['nuclei']['centroid_x'], v['nuclei']['centroid_y']], 1)
                            save_cell_graph(opt.graph_file, cg, xy=xy, labels=v.get('labels'))
                            print(f'cell graph written to {opt.graph_file}')
                    if opt.texture:
                        torch.cuda.synchronize()
                        t0 = time.time()
                        tx = slide_nucleus_texture(v, slide, stain=opt.texture, matrix=est.matrix if est is not None else None)
                        torch.cuda.synchronize()
                        dtt = (time.time() - t0) * 1e3
                        held = ~torch.isnan(tx['tex_contrast_mean'])
                        medt = lambda c: float(c[held].median()) if bool(held.any()) else float('nan')
                        print(f'texture {opt.slide}x{opt.slide}, task {k}: {int(held.sum())} nuclei textured on {opt.texture}, median contrast '
                              f'{medt(tx["tex_contrast_mean"]):.3f}, median entropy {medt(tx["tex_entropy_mean"]):.3f} in {dtt:.2f} ms')
                        v['nuclei'].update(tx)
                    if opt.table:
                        save_nucleus_table(opt.table, v['nuclei'])
                        print(f'nucleus table written to {opt.table}')
        if opt.score:
            # synthetic weights detect nothing meaningful, so the scored detections are synthetic too: annotations at nucleus density and
            # detections made from them (synth.synth_slide_truth)
            n_obj = max(1, int((opt.slide / 40.0) ** 2))
            tb, tl, pb, ps, pl = (torch.from_numpy(a).to(device) for a in synth.synth_slide_truth(n_obj, opt.slide, opt.nc, seed=5))
            info = {}
            torch.cuda.synchronize()
            t0 = time.time()
            st = score_slide({'boxes': pb, 'scores': ps, 'labels': pl}, {'boxes': tb, 'labels': tl}, info=info)
            torch.cuda.synchronize()
            print(f'score: {len(ps)} detections x {len(tl)} truths, mAP@.5 {float(st["ap"][:, 0].mean()):.4f}, chunk pairs visited / total '
                  f'{info["chunks_visited"]} / {info["chunks_total"]} ({info["chunks_visited"] / max(info["chunks_total"], 1):.4f}) in {(time.time() - t0) * 1e3:.1f} ms')
            if opt.masks and opt.label_map:
                # the same synthetic sets as segmentations: one fixed disc pasted into every box (no rasteriser of its own), detections in
                # descending score order so that the best one owns a contested pixel
                from hd_yolo_amd import ops
                yy, xx = torch.meshgrid(torch.arange(28, device=device), torch.arange(28, device=device), indexing='ij')
                disc = (((yy - 13.5) ** 2 + (xx - 13.5) ** 2) <= 13.5 ** 2).float()
                order = torch.sort(ps, descending=True, stable=True)[1]
                size = (opt.slide, opt.slide)
                truth_map = ops.paste_label_map(disc.expand(len(tl), 28, 28), tb, size)
                pred_map = ops.paste_label_map(disc.expand(len(ps), 28, 28), pb[order], size)
                torch.cuda.synchronize()
                t0 = time.time()
                sm = score_slide_masks({'label_map': pred_map, 'scores': ps[order], 'labels': pl[order]}, {'label_map': truth_map, 'labels': tl})
                torch.cuda.synchronize()
                print(f'mask score: {len(ps)} detections x {len(tl)} truths on a {opt.slide} x {opt.slide} label map, {len(sm["pairs"])} overlapping pairs, '
                      f'mask mAP@.5 {float(sm["ap"][:, 0].mean()):.4f} in {(time.time() - t0) * 1e3:.1f} ms')
                seg = slide_segmentation_summary(sm, pl[order], tl, nc=opt.nc)
                print(f'mask summaries: PQ {seg["pq"]:.4f} SQ {seg["sq"]:.4f} DQ {seg["dq"]:.4f} mPQ {seg["mpq"]:.4f} AJI {seg["aji"]:.4f} Dice {seg["dice"]:.4f} '
                      f'(tp {seg["tp"]} fp {seg["fp"]} fn {seg["fn"]})')


if __name__ == '__main__':
    main()
