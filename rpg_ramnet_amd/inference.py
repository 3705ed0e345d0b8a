"""Streaming inference and offline evaluation drivers: the counterparts of the hot loop of ``RAM_Net/test.py:205-395``
and of the file pairing / aggregation of ``RAM_Net/evaluation.py:295-397``.

test.py's contract: batch 1, ONE data package per model call, the recurrent state lives in the objects the
model returns and is fed back on the next call; it is reset whenever the dataset index of ``ConcatDatasetCustom``
increases (a new recording); the first two packages of every recording are not saved ("such that the temporal
dependencies of the network are settled").  Written files (the layout evaluation.py globs):

    <out>/npy/<key>/depth_{idx:010d}.npy                      prediction, normalised log depth, float32 [1, H, W]
    <out>/ground_truth/npy/depth_<key>/frame_{idx:010d}.npy   target, same encoding
and, with ``images=True``, test.py's pictures of the same packages (test.py:259-360; rendered on the device by ``render``):
    <out>/depth/<key>/frame_{idx:010d}.png                          prediction * 255, greyscale
    <out>/color_map/<key>/frame_{idx:010d}.png                      prediction through make_colormap and the run's colour mapper, RGBA
    <out>/ground_truth/grey/depth_<key>/frame_{idx:010d}.png        the same two of the target
    <out>/ground_truth/color_map/depth_<key>/frame_{idx:010d}.png
    <out>/video/predictions|gt|inputs/frame_{video_idx:010d}.png    colour maps again and the input previews (events red / blue, the frame
                                                                    grey), one per key of test.py's video list, numbered through the run
"""
import glob
import os
from os.path import join

import numpy as np
import torch

from .metrics import EVAL_CUTOFFS, EvalTable, depth_metrics

TEST_METRICS = ("mse", "abs_rel_diff", "scale_invariant_error", "median_error", "mean_error", "rms_linear")      # test.py:27, in its order


def empty_states(every_x_rgb_frame):
    """State dictionaries of a fresh recording (test.py:215-222)."""
    lstm = {}
    for k in range(every_x_rgb_frame):
        lstm['events{}'.format(k)] = None
        lstm['depth{}'.format(k)] = None
    lstm['image'] = None
    return {'image': None}, lstm


def _is_model_input(key, value):
    return torch.is_tensor(value) and value.is_floating_point() and (key == "image" or (key.startswith("events") and key[6:].isdigit()))


def input_gradients(model, sequence, loss_composition, loss_weights=None, **loss_kwargs):
    """Attribution: the gradient of trainer.sequence_loss with respect to every event grid and frame of `sequence` (a list of packages
    as the trainers feed them, 'depth_<key>' targets included), with the weights held fixed.

    Every parameter's requires_grad is switched off for the call and restored afterwards (also when the loss raises), every
    `events<k>` / `image` tensor enters as a leaf of its own (the caller's tensors are not touched), and one backward pass runs: no
    parameter's .grad is read or written and no backward-weights kernel is launched — the backward-data launches alone, down to the
    head layers (ramnet_head_dgrad) and the input repack.  loss_weights: one weight per key of loss_composition (default: ones);
    loss_kwargs: the further arguments of trainer.sequence_loss (loss_params, grad_loss_weight, loss_type, mse_loss).
    Returns (loss, [{key: gradient} per package]): the detached loss and NCHW gradients of the shape, dtype and device of what was
    passed (zeros for an input the model did not read).  First derivatives only; captured graphs are not involved."""
    from .trainer import sequence_loss
    if loss_weights is None:
        loss_weights = [1.0] * len(loss_composition or ())
    params = [p for p in model.parameters()]
    flags = [p.requires_grad for p in params]
    try:
        for p in params:
            p.requires_grad_(False)
        leaves, seq = [], []
        for item in sequence:
            mine = {k: v.detach().requires_grad_(True) for k, v in item.items() if _is_model_input(k, v)}
            leaves.append(mine)
            seq.append(dict(item, **mine))
        with torch.enable_grad():
            total, _ = sequence_loss(model, seq, loss_composition, loss_weights, **loss_kwargs)
            total.backward()
        grads = [{k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in mine.items()} for mine in leaves]
        return total.detach(), grads
    finally:
        for p, f in zip(params, flags):
            p.requires_grad_(f)


def _time_batched_ok(model):
    return (type(model).__name__ == "ERGB2DepthRecurrent" and not bool(model.baseline) and model.recurrent_block_type == "conv"
            and torch.device(model.gpu).type == "cuda")


def video_keys(model, every_x_rgb_frame):
    """The keys test.py draws into video/ (test.py:318-326)."""
    baseline = getattr(model, "baseline", False)
    if baseline == "rgb" or type(model).__name__ == "ERGB2Depth":
        return ["image"]
    keys = ["events{}".format(i) for i in range(every_x_rgb_frame - 1)]
    if not baseline:
        keys.append("events{}".format(every_x_rgb_frame - 1))
    return keys + ["image"]


def _write_images(R, output_folder, idx, video_idx, pkeys, tkeys, vkeys, color, grey, rgb):
    """test.py:262-360 for one package from the planes of render.render_package (host arrays); returns the next video index."""
    name = 'frame_{:010d}.png'.format(idx)
    for j, key in enumerate(pkeys + tkeys):
        gdir, cdir = ("depth", "color_map") if j < len(pkeys) else ("ground_truth/grey", "ground_truth/color_map")
        for d, plane in ((join(output_folder, gdir, key), grey[j]), (join(output_folder, cdir, key), color[j])):
            os.makedirs(d, exist_ok=True)
            R.write_png(join(d, name), plane)
    for j, key in enumerate(vkeys):
        name = 'frame_{:010d}.png'.format(video_idx)
        for sub, plane in (("predictions", color[pkeys.index(key)]), ("gt", color[len(pkeys) + tkeys.index("depth_" + key)]), ("inputs", rgb[j])):
            d = join(output_folder, "video", sub)
            os.makedirs(d, exist_ok=True)
            R.write_png(join(d, name), plane)
        video_idx += 1
    return video_idx


def stream_dataset(model, dataset, every_x_rgb_frame, output_folder=None, settle=2, calculate_scale=False,
                   reg_factor=5.70378, clip_distance=1000.0, max_items=None, time_batched="auto", table=None, rescale=False,
                   images=False, color_mapper=None, metrics=False):
    """Run ``model`` over ``dataset`` (items ``(sequence, dataset_idx)``, sequence_length 1) the way test.py does and
    optionally write predictions / targets as .npy.  Returns {'items', 'saved', 'scale': (mean, min, max) or None}.

    time_batched ("auto" = whenever the model allows it): a data package IS one group of ``graph.TimeBatchedStream`` — its K event
    grids encode at batch K, its K + 1 decodes run as one chain, only the state updates are sequential — with the same outputs
    bit for bit; False calls ``model(package, ...)`` as test.py:230-232 does.

    table: a dict prediction key -> ``metrics.EvalTable``, or True to create one per prediction key from ``clip_distance`` /
    ``reg_factor``: every package past ``settle`` adds each prediction with its ``depth_<key>`` target to that key's table while it is
    still on the device — no ``output_folder`` and no read-back inside the loop; the tables come back under ``info["tables"]``.
    rescale: the tables that ``table=True`` creates are rescaled ones (evaluation.py's --rescale).

    images (with ``output_folder``): every saved package also gets test.py's pictures (the module docstring lists them): ONE call of
    ``render.render_package`` and ONE device-to-host copy of its uint8 planes per package.  color_mapper: the ``render.ColorMapper`` of
    the run; None builds it as test.py does, from the target of package 20 (``ColorMapper.from_target``).  The .npy files do not change.
    calculate_scale="device": the same (mean, min, max) from ``render.least_squares_scale`` (float64 sums on the device; it rides in the
    render call of a drawn package), one read-back after the loop; True keeps the float32 host path of test.py:365-378.
    metrics: ``info["total_metrics"]`` = test.py:394, the mean over every package past ``settle`` and every key of TEST_METRICS (test.py's
    six, in its order) from ``metrics.batch_metrics``, one read-back after the loop (None when there was no such package).
    With any of the three the package is moved to the model's device once, and model, renderer and metrics read that copy."""
    tables = {} if table is True else table
    use_tb = _time_batched_ok(model) if time_batched == "auto" else bool(time_batched)
    tb, K = None, every_x_rgb_frame
    n = len(dataset) if max_items is None else min(len(dataset), max_items)
    device_scale = isinstance(calculate_scale, str) and calculate_scale == "device"
    if isinstance(calculate_scale, str) and not device_scale:
        raise ValueError("stream_dataset: calculate_scale is False, True or \"device\", got %r" % (calculate_scale,))
    host_scale = bool(calculate_scale) and not device_scale
    scale = np.empty(n) if host_scale else None
    draw = bool(images) and bool(output_folder)
    device = torch.device(model.gpu) if (draw or device_scale or metrics) else None
    R, vkeys, video_idx, device_scales, metric_rows = None, [], 0, [], []
    if draw or device_scale:
        from . import render as R
    if draw:
        if color_mapper is None:
            if len(dataset) <= 20:
                raise ValueError("stream_dataset: images=True takes its colour mapper from package 20 (test.py:197), the dataset has %d; "
                                 "pass color_mapper=" % len(dataset))
            color_mapper = R.ColorMapper.from_target(dataset[20][0][0]['depth_image'])
        vkeys = video_keys(model, every_x_rgb_frame)
    if metrics:
        from .metrics import batch_metrics
    saved = 0
    was_training = model.training
    model.eval()
    with torch.no_grad():
        prev_dataset_idx = -1
        for idx in range(n):
            item, dataset_idx = dataset[idx]
            if dataset_idx > prev_dataset_idx:
                prev_super, prev_lstm = empty_states(every_x_rgb_frame)
                sequence_idx = 0
            package = {k: v[None, :] for k, v in item[0].items()}
            if device is not None:                                  # moved once: the model, the renderer and the metrics read this copy
                package = {k: v.to(device, non_blocking=True) for k, v in package.items()}
            if use_tb:
                hw = tuple(package['image'].shape[2:])
                if tb is None or (tb.H, tb.W) != hw:                # a ConcatDatasetCustom may mix recordings of different resolution:
                    from .graph import TimeBatchedStream          # the runtime's static buffers are per resolution -> a new one
                    tb = TimeBatchedStream(model, 1, hw[0], hw[1], max_events=K + 1)
                if sequence_idx == 0:
                    tb.reset()                                    # a new recording starts from the zero state
                for k in range(K):
                    tb.push_events(package['events{}'.format(k)])
                out = tb.wait(tb.push_image(package['image']))    # [K + 1, 1, 1, H, W]: views of a static buffer, valid until the second-next
                #                                                   group of this shape (they are written to disk right below)
                preds = {'events{}'.format(k): out[k] for k in range(K)}
                preds['image'] = out[K]
                new_super, new_lstm = prev_super, prev_lstm        # (the runtime carries the state)
            else:
                preds, new_super, new_lstm = model(package, prev_super['image'], prev_lstm)
            if output_folder and sequence_idx >= settle:
                for key, img in preds.items():
                    d = join(output_folder, "npy", key)
                    os.makedirs(d, exist_ok=True)
                    np.save(join(d, 'depth_{:010d}.npy'.format(idx)), img[0].cpu().numpy())
                for key, value in package.items():
                    if 'depth' in key:
                        d = join(output_folder, "ground_truth/npy", key)
                        os.makedirs(d, exist_ok=True)
                        np.save(join(d, 'frame_{:010d}.npy'.format(idx)), value[0].cpu().numpy())
                saved += 1
            if device is not None:
                pkeys = list(preds)
                pairs = ([preds[k] for k in pkeys], [package['depth_' + k] for k in pkeys])
            if draw and sequence_idx >= settle:
                tkeys = [k for k in package if 'depth' in k]
                maps = pairs[0] + [package[k] for k in tkeys]
                buf, _, _, _, s = R.render_package(maps, color_mapper, [package[k] for k in vkeys], vkeys,
                                                   scale=pairs + (clip_distance, reg_factor) if device_scale else None)
                color, grey, rgb = R.split_package(buf.cpu().numpy(), len(maps), len(vkeys), tuple(maps[0].shape[-2:]))
                video_idx = _write_images(R, output_folder, idx, video_idx, pkeys, tkeys, vkeys, color, grey, rgb)
            elif device_scale:
                s = R.least_squares_scale(pairs[0], pairs[1], clip_distance, reg_factor)
            if device_scale:
                device_scales.append(s[-1:])                        # (the last key wins, as on the host path)
            if metrics and sequence_idx >= settle:
                metric_rows.append(batch_metrics(pairs[0], pairs[1], TEST_METRICS))
            if tables is not None and sequence_idx >= settle:
                for key, img in preds.items():
                    if key not in tables:
                        if table is not True:
                            continue
                        tables[key] = EvalTable(clip_distance, reg_factor, rescale=rescale)
                    tables[key].add([img[0]], [package['depth_' + key][0]])      # (launched now: img is a view of a static buffer)
            if host_scale:           # least-squares scale between metric prediction and target (test.py:365-378; last key wins there, too)
                for key, img in preds.items():
                    p = np.exp(reg_factor * (img[0][0].cpu().numpy() - np.float32(1.0))) * clip_distance
                    t = np.exp(reg_factor * (package['depth_' + key][0][0].cpu().numpy() - np.float32(1.0))) * clip_distance
                    scale[idx] = np.sum(p * t) / np.sum(p * p)
            prev_super, prev_lstm = new_super, new_lstm
            sequence_idx += 1
            prev_dataset_idx = dataset_idx
    model.train(was_training)
    if device_scale:
        scale = torch.cat(device_scales).cpu().numpy() if device_scales else np.empty(0)         # the one read-back
    info = {"items": n, "saved": saved,
            "scale": (float(np.mean(scale)), float(np.min(scale)), float(np.max(scale))) if calculate_scale else None}
    if metrics:
        rows = torch.cat(metric_rows).cpu().numpy() if metric_rows else None                       # the one read-back
        info["total_metrics"] = None if rows is None else np.sum(rows, 0) / len(rows)
    if tables is not None:
        info["tables"] = tables
    return info


def evaluate_folders(predictions_dir, targets_dir, clip_distance, reg_factor, crop_ymax=None, prediction_offset=0,
                     target_offset=0, cutoffs=(10, 20, 30, 80, 250, 500), device="cuda:0"):
    """evaluation.py:295-397 on device: sorted ``*.npy`` of both folders are paired by position, rows ``[:crop_ymax]`` kept,
    both converted to metric depth, per-file metrics averaged over files — for all pixels and for every depth cut-off
    (keys ``"<cutoff>_<metric>"``).  Files without a valid pixel inside a cut-off are skipped for that cut-off."""
    p_files = sorted(glob.glob(join(predictions_dir, '*.npy')))[prediction_offset:]
    t_files = sorted(glob.glob(join(targets_dir, '*.npy')))[target_offset:]
    assert len(p_files) > 0 and len(t_files) > 0
    sums, counts = {}, {}
    for p_file, t_file in zip(p_files, t_files):
        t, p = np.load(t_file)[0], np.load(p_file)[0]
        if crop_ymax is not None:
            t, p = t[:crop_ymax], p[:crop_ymax]
        assert p.shape == t.shape
        pt, tt = torch.from_numpy(p).to(device), torch.from_numpy(t).to(device)
        for cut in (None,) + tuple(cutoffs):
            m = depth_metrics(pt, tt, clip_distance, reg_factor, cutoff=float("inf") if cut is None else float(cut))
            if m.get("n", 0) == 0:
                continue
            pre = "" if cut is None else "%d_" % cut
            for k, v in m.items():
                if k != "n":
                    sums[pre + k] = sums.get(pre + k, 0.0) + v
            counts[pre] = counts.get(pre, 0) + 1
    out = {k: v / counts[k.split("_")[0] + "_" if k.split("_")[0].isdigit() else ""] for k, v in sums.items()}
    out["files"] = len(p_files)
    return out


def evaluate_table(predictions_dir, targets_dir, clip_distance, reg_factor, crop_ymax=None, prediction_offset=0, target_offset=0,
                   cutoffs=EVAL_CUTOFFS, event_masks_dir=None, batch_files=64, skip_empty=True, device="cuda:0", rescale=False,
                   down_scale_factor=1.0):
    """evaluation.py:295-397 with the whole table on the device: the file pairing of ``evaluate_folders``, ``batch_files`` files at a time
    into one ``metrics.EvalTable`` (three launches per batch, one read-back at the end), all ten metrics for all pixels and every cut-off.
    event_masks_dir: the sorted ``*png`` event frames of that folder, from ``prediction_offset`` on, give the ``event_masked_*`` half of the
    table (mask = ``sum(frame.astype(float32), -1) > 0``, cropped like the maps; evaluation.py:371-390).
    skip_empty: ``evaluate_folders``' rule (True) or the reference's sum / number of files (False), see ``metrics.finish_eval_rows``.
    rescale / down_scale_factor: evaluation.py's --rescale and --down_scale_factor, see ``metrics.EvalTable``; ``crop_ymax`` is applied to
    every map first, as the reference does, and event frames must already have the size of the predictions."""
    p_files = sorted(glob.glob(join(predictions_dir, '*.npy')))[prediction_offset:]
    t_files = sorted(glob.glob(join(targets_dir, '*.npy')))[target_offset:]
    assert len(p_files) > 0 and len(t_files) > 0
    pairs = list(zip(p_files, t_files))
    e_files = None
    if event_masks_dir is not None:
        from .data import _imread
        e_files = sorted(glob.glob(join(event_masks_dir, '*png')))[prediction_offset:]
        assert len(e_files) >= len(pairs), "%d event frames for %d file pairs" % (len(e_files), len(pairs))
    tab = EvalTable(clip_distance, reg_factor, cutoffs, rescale=rescale, down_scale_factor=down_scale_factor)
    same_size = down_scale_factor >= 1.0
    for i0 in range(0, len(pairs), batch_files):
        ps, ts, ms = [], [], []
        for i in range(i0, min(i0 + batch_files, len(pairs))):
            t, p = np.load(pairs[i][1])[0], np.load(pairs[i][0])[0]
            if crop_ymax is not None:
                t, p = t[:crop_ymax], p[:crop_ymax]
            assert p.shape == t.shape or not same_size
            ps.append(p), ts.append(t)
            if e_files is not None:
                frame = _imread(e_files[i])
                frame = frame[:crop_ymax] if crop_ymax is not None else frame
                m = np.sum(frame.astype("float32").reshape(frame.shape[:2] + (-1,)), axis=-1) > 0
                assert m.shape == t.shape or not same_size      # (a down-scaled table checks the masks against the predictions itself)
                ms.append(m)
        if len(set(p.shape for p in ps)) == 1 and len(set(t.shape for t in ts)) == 1:                      # one upload per batch
            tab.add(torch.from_numpy(np.stack(ps)).to(device), torch.from_numpy(np.stack(ts)).to(device),
                    torch.from_numpy(np.stack(ms)).to(device) if e_files is not None else None)
        else:                                                       # (recordings of different resolution in one folder: one call per file)
            for j in range(len(ps)):
                tab.add(torch.from_numpy(ps[j][None]).to(device), torch.from_numpy(ts[j][None]).to(device),
                        torch.from_numpy(ms[j][None]).to(device) if e_files is not None else None)
    out = tab.result(skip_empty=skip_empty)
    out["files"] = len(p_files)
    return out
