"""Sequence-level driver: the call pattern and loss assembly of the reference's
LSTMTrainer.forward_pass_sequence (RAM_Net/trainer/lstm_trainer.py:228-390, :152-226) around the HIP model.

Quirk mirrored: the reference aliases ONE loss dict for every supervised key and adds the second key's
total under no_grad, so the DIFFERENTIATED scalar is (sum_{l,key} w_key SI)/L while the REPORTED loss is that value
times the number of supervised keys.  `sequence_loss` returns both.
"""
import torch

from . import ops


def empty_states_lstm(K):
    d = {}
    for k in range(K):
        d['events{}'.format(k)] = None
        d['depth{}'.format(k)] = None
    d['image'] = None
    return d


def freeze(model, patterns, train_only=False):
    """Partial training by the ordinary idiom: sets requires_grad = False on parameters of `model` picked by `patterns`, fnmatch
    patterns (a string or a list of them) over the names of model.named_parameters(), and returns the names it froze, in
    registration order.  train_only=False: the matching tensors are frozen.  train_only=True: the patterns name what stays trainable
    and EVERY OTHER tensor is frozen.  A pattern that matches no name raises KeyError (a typo must not train, or freeze, the whole
    network silently).  Nothing is ever un-frozen here (`p.requires_grad_(True)` does that), so calls compose.  The operators read the
    flags at every pass: a frozen tensor gets no .grad, its backward-weights launches and folds are skipped, and gradients still flow
    through its layer ("Partial training")."""
    import fnmatch
    patterns = [patterns] if isinstance(patterns, str) else list(patterns)
    named = list(model.named_parameters())
    hit = set()
    for pat in patterns:
        m = [n for n, _ in named if fnmatch.fnmatchcase(n, pat)]
        if not m:
            raise KeyError("freeze: pattern %r matches no parameter name (e.g. %s)" % (pat, ", ".join(n for n, _ in named[:3])))
        hit.update(m)
    frozen = []
    for n, p in named:
        if (n in hit) != bool(train_only):
            p.requires_grad_(False)
            frozen.append(n)
    return frozen


def apply_freeze_config(model, config):
    """The optional keys config['trainer']['freeze'] / config['trainer']['train_only'] (lists of patterns for `freeze`; absent = every
    tensor trains): applied by the trainers BEFORE they build an optimizer — and to be called before a parallel.FlatGradReducer or a
    graph.GraphedTrainStep is built, whose layouts follow the flags.  Idempotent.  Returns the frozen names."""
    tr = config.get('trainer', {})
    frozen = []
    if tr.get('freeze'):
        frozen += freeze(model, tr['freeze'])
    if tr.get('train_only'):
        frozen += freeze(model, tr['train_only'], train_only=True)
    return frozen


LOSS_SEMANTICS = {
    False: "per-rank mean over the rank's batch, gradients averaged over ranks (standard DDP)",
    True: "exact global batch: SI statistics (sum d, sum d^2, n per supervised map) all-reduced before the backward; the N-rank "
          "gradient equals the single-rank gradient on the concatenated batch (model/loss.py:9)",
}


def apply_deterministic_config(config):
    """The optional key config['trainer']['deterministic'] (default false; not in the reference): true switches the deterministic mode on
    (ops.set_deterministic) for the process — bit-reproducible steps per rank on the same machine, device, world size and library build;
    the order in which a collective sums the ranks' gradients is the communication library's.  Absent or false leaves the switch alone."""
    if config.get('trainer', {}).get('deterministic', False):
        ops.set_deterministic(True)
    return ops.deterministic()


LOSS_TYPES = ("scale_invariant_loss", "scale_invariant_log_loss", "mse_loss")      # config['loss']['type'] (train.py:192 getattr(module_loss, ...))


def _nominal_loss(loss_type, value, target, loss_params):
    if loss_type == "scale_invariant_loss":
        return ops.scale_invariant_loss(value, target, **loss_params)
    if loss_type == "scale_invariant_log_loss":
        return ops.scale_invariant_log_loss(value, target, **{k: v for k, v in loss_params.items() if k == "n_lambda"})
    if loss_type == "mse_loss":
        return ops.mse_loss(value, target)
    raise KeyError(loss_type)


def sequence_loss(model, sequence, loss_composition, loss_weights, loss_params=None, grad_loss_weight=None, dp_exact=False,
                  process_group=None, loss_type="scale_invariant_loss", mse_loss=None, parts=False):
    """BPTT over the L packages of `sequence` (list of item dicts with 'depth_<key>' targets).
    grad_loss_weight: weight of the multi-scale gradient loss (config['grad_loss']['weight'], 0.25 in the released
    recipe; lstm_trainer.py:162-168, :197-199) or None for the SI loss alone.
    dp_exact (data parallel; default off): the reference's loss takes mean(d)^2 over the WHOLE batch (model/loss.py:9),
    which an average of per-rank losses is not.  With dp_exact every rank computes (sum d, sum d^2, n) of each of its supervised
    maps, ONE all-reduce sums the [terms x 4] table over the ranks before the backward, and every term's value and gradient follow
    from the global sums (ops.SILossFromStats) — after the reducer's gradient average the N-rank gradient is the single-rank one on
    the concatenated batch, and every rank reports the global loss.  The multi-scale gradient loss normalises every scale by its own
    count of valid components: its per-scale (sum |g|, count) statistics ride in the same table and all-reduce, and its value and
    gradient follow from the global sums and the global batch count (ops.MSGLossBatchFromStats).
    The gradient loss of all supervised maps is ONE batched call after the forward loop (ops.multi_scale_grad_loss_batch; one per
    distinct map shape) unless ops.set_grad_loss_batched(False) restores one call per map.
    loss_type: config['loss']['type'] — 'scale_invariant_loss' (every shipped config), 'scale_invariant_log_loss' (model/loss.py:12-15)
    or 'mse_loss' (:18-19); loss_params = config['loss']['config'].
    mse_loss: config['mse_loss'] (lstm_trainer.py:76-90) — {'weight': 1.0, 'downsampling_factor': 0.5} — adds
    weight * sum_terms w_key * mse(bilinear x factor of prediction and target) / L (lstm_trainer.py:169-185, :205-208), or None.
    Returns (loss to call .backward() on, loss value the reference would report).
    parts=True: a third value, the dict `loss_parts` describes plus 'predictions': [(package index, key, detached prediction)] of EVERY
    key the model returned (what the reference's calculate_total_metrics loop sees, lstm_trainer.py:290-294)."""
    if loss_params is None:
        loss_params = {"weight": 1.0, "n_lambda": 1.0} if loss_type == "scale_invariant_loss" else {}
    if dp_exact:
        assert loss_type == "scale_invariant_loss" and mse_loss is None, "dp_exact: the scale-invariant loss only"
        if any('num_events' in it for it in sequence):
            raise NotImplementedError("dp_exact: batches of irregular packages (num_events) are not supported")
        if parts:
            raise NotImplementedError("dp_exact: parts=True is not supported")
        return _sequence_loss_dp_exact(model, sequence, loss_composition, loss_weights, loss_params, grad_loss_weight, process_group)
    gterms, mterms, gtriples = [], [], []
    gbatched = grad_loss_weight is not None and ops.grad_loss_batched()
    L = len(sequence)
    assert L > 0
    K = model.every_x_rgb_frame
    prev_super, prev_lstm = None, empty_states_lstm(K)
    terms, keys_seen, seen = [], [], []
    # the scale-invariant loss of the supervised predictions inside the prediction layer's own launches (ops.PredSigmoidSI): the model is
    # told which keys and parameters for the duration of its forward call and hangs the loss term on the prediction it returns
    si_par = (float(loss_params.get("weight", 1.0)), float(loss_params.get("n_lambda", 1.0))) if loss_type == "scale_invariant_loss" else None
    ask = si_par is not None and ops.si_fusion() and isinstance(loss_composition, (list, tuple)) and hasattr(model, "_si_request")
    for l, item in enumerate(sequence):
        if ask:
            model._si_fuse = {"weight": si_par[0], "n_lambda": si_par[1], "keys": list(loss_composition)}
            # the supervised targets move to the device ONCE (a DataLoader item holds CPU tensors): the model's fused loss and the term below
            # then see the same tensor — a second copy would make the pointers differ, the fused term be dropped and its launches wasted
            moved = {}
            for key in loss_composition:
                t = item.get('depth_' + key)
                if torch.is_tensor(t) and (t.device != torch.device(model.gpu) or t.dtype != torch.float32 or not t.is_contiguous()):
                    moved['depth_' + key] = t.to(device=model.gpu, dtype=torch.float32).contiguous()
            if moved:
                item = dict(item, **moved)
        try:
            preds, supers, lstms = model(item, prev_super, prev_lstm)
        finally:
            if ask:
                model._si_fuse = None
        for key, value in preds.items():
            if parts:
                seen.append((l, key, value.detach()))
            if not loss_composition or key in loss_composition:
                w = loss_weights[loss_composition.index(key)]
                target = item['depth_' + key].to(model.gpu)
                fused = getattr(value, "_si_fused", None)
                if fused is not None and ask and fused[2] == si_par and target.dtype == torch.float32 and fused[1] == target.data_ptr():
                    terms.append(w * fused[0])
                else:
                    terms.append(w * _nominal_loss(loss_type, value, target, loss_params))
                if gbatched:
                    gtriples.append((w, value, target))
                elif grad_loss_weight is not None:
                    gterms.append(w * ops.multi_scale_grad_loss(value, target))
                if mse_loss is not None:
                    mterms.append(w * ops.mse_loss(value, target, mse_loss.get('downsampling_factor', 0.5)))
                if key not in keys_seen:
                    keys_seen.append(key)
        prev_super, prev_lstm = supers['image'], lstms
    total = si = torch.stack(terms).sum() / float(L)
    gl = ml = None
    if gbatched:
        gl = grad_loss_weight * _batched_grad_loss(gtriples) / float(L)
        total = total + gl
    elif grad_loss_weight is not None:
        gl = grad_loss_weight * torch.stack(gterms).sum() / float(L)
        total = total + gl
    if mse_loss is not None:
        ml = float(mse_loss.get('weight', 1.0)) * torch.stack(mterms).sum() / float(L)
        total = total + ml
    if parts:
        return total, total.detach() * len(keys_seen), dict(loss_parts(len(keys_seen), total, si, gl, ml), predictions=seen)
    return total, total.detach() * len(keys_seen)


def _by_shape(triples):
    """(w, prediction, target) triples grouped by map shape, in order of first appearance (every shipped configuration: one group)."""
    groups = {}
    for tr in triples:
        groups.setdefault(tuple(tr[1].shape), []).append(tr)
    return list(groups.values())


def _batched_grad_loss(triples):
    """sum of w x multi_scale_grad_loss over the supervised (w, prediction, target) triples: one batched call per distinct map shape."""
    sums = [ops.multi_scale_grad_loss_batch([v for _, v, _ in grp], [t for _, _, t in grp], [w for w, _, _ in grp], with_sum=True)[1]
            for grp in _by_shape(triples)]
    return sums[0] if len(sums) == 1 else torch.stack(sums).sum()


def loss_parts(n_keys, total, si, grad=None, mse=None):
    """The reference's `total_batch_losses` (lstm_trainer.py:189-226, :381-383): calculate_total_batch_loss runs once per supervised key
    on the ONE aliased loss dict, so EVERY entry — 'loss', 'L_si', and 'L_grad' / 'L_mse' when configured — is (#supervised keys) x the
    differentiated part.  Detached tensors; nothing is read back."""
    out = {'loss': total.detach() * n_keys, 'L_si': si.detach() * n_keys}
    if grad is not None:
        out['L_grad'] = grad.detach() * n_keys
    if mse is not None:
        out['L_mse'] = mse.detach() * n_keys
    return out


def _sequence_loss_dp_exact(model, sequence, loss_composition, loss_weights, loss_params, grad_loss_weight, group):
    import torch.distributed as dist
    L = len(sequence)
    assert L > 0
    K = model.every_x_rgb_frame
    prev_super, prev_lstm = None, empty_states_lstm(K)
    sup, gterms, keys_seen = [], [], []
    gbatched = grad_loss_weight is not None and ops.grad_loss_batched()
    for item in sequence:
        preds, supers, lstms = model(item, prev_super, prev_lstm)
        for key, value in preds.items():
            if not loss_composition or key in loss_composition:
                w = loss_weights[loss_composition.index(key)]
                target = item['depth_' + key].to(model.gpu).float()
                sup.append((w, value.float(), target))
                if grad_loss_weight is not None and not gbatched:
                    gterms.append(w * ops.multi_scale_grad_loss(value, target))
                if key not in keys_seen:
                    keys_seen.append(key)
        prev_super, prev_lstm = supers['image'], lstms
    # [terms x 4 SI sums | per shape group: pairs x 4 scales x (sum |g|, count) | local batch count]: ONE all-reduce for everything
    groups = _by_shape(sup) if gbatched else []
    nsi = 4 * len(sup)
    flat = torch.empty(nsi + (sum(8 * len(grp) for grp in groups) + 1 if gbatched else 0), device=model.gpu, dtype=torch.float64)
    table = flat[:nsi].view(len(sup), 4)
    for i, (_, value, target) in enumerate(sup):
        ops.si_local_stats(value.detach(), target, table[i])
    gstats, o = [], nsi
    for grp in groups:
        gstats.append(ops.msg_local_stats([v for _, v, _ in grp], [t for _, _, t in grp], out=flat[o:o + 8 * len(grp)].view(len(grp), 4, 2)))
        o += 8 * len(grp)
    if gbatched:
        flat[-1] = float(sup[0][1].shape[0])
    world = 1
    if dist.is_available() and dist.is_initialized():
        world = dist.get_world_size(group)
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)        # stream-ordered on the compute stream: 32 B per term, 96 B with the gradient loss
    terms = [w * ops.SILossFromStats.apply(value, target, table[i], float(loss_params["weight"]), float(loss_params["n_lambda"]),
                                           float(world)) for i, (w, value, target) in enumerate(sup)]
    total = torch.stack(terms).sum() / float(L)
    if gbatched:
        # the global batch count (the sum of the ranks' B) is the last entry of the reduced table: the kernels read it on the device
        sums = [ops.multi_scale_grad_loss_from_stats([v for _, v, _ in grp], [t for _, _, t in grp], g, flat[-1:], gain=float(world),
                                                     weights=[w for w, _, _ in grp], with_sum=True)[1] for grp, g in zip(groups, gstats)]
        total = total + grad_loss_weight * (sums[0] if len(sums) == 1 else torch.stack(sums).sum()) / float(L)
    elif grad_loss_weight is not None:
        total = total + grad_loss_weight * torch.stack(gterms).sum() / float(L)
    # value: SILossFromStats.forward returns the global loss itself (the gain only scales its backward)
    return total, total.detach() * len(keys_seen)


class EpochTrainer:
    """Epoch-level half of the reference trainer (RAM_Net/base/base_trainer.py:16-61 constructor, :65-123 `train`, :133-158
    `_save_checkpoint`, :160-179 `_resume_checkpoint`) around a user-supplied epoch function — NOT the control plane: no
    TensorBoard, no previews, no metric plumbing.

    config keys used exactly as the reference reads them: 'name', 'optimizer_type' + 'optimizer', 'lr_scheduler_type' +
    'lr_scheduler' + 'lr_scheduler_freq', config['trainer']: 'epochs', 'save_freq', 'save_dir', 'monitor', 'monitor_mode'.
    ``train_epoch(epoch) -> dict`` returns the epoch's log entries (at least 'loss' and the monitored key).  Order of events per
    epoch, as in base_trainer.py:103-122: log entry -> best-checkpoint (saved under the epoch name, then renamed to
    'model_best.pth.tar') -> periodic checkpoint when epoch % save_freq == 0 -> scheduler step when epoch % lr_scheduler_freq == 0.
    Checkpoints have the reference's dict layout (checkpoint.save_checkpoint)."""

    def __init__(self, model, config, train_epoch, resume=None, train_logger=None, reducer=None):
        import math
        import os
        from . import checkpoint as ck
        self.model, self.config, self.train_epoch, self.reducer = model, config, train_epoch, reducer
        apply_deterministic_config(config)
        self.epochs = config['trainer']['epochs']
        self.save_freq = config['trainer']['save_freq']
        # optional partial training (config['trainer']['freeze' | 'train_only']) BEFORE the optimizer exists; the optimizer still gets
        # model.parameters() as the reference's does — it skips tensors without .grad, and checkpoints keep the reference layout
        self.frozen = apply_freeze_config(model, config)
        self.optimizer = getattr(torch.optim, config['optimizer_type'])(model.parameters(), **config['optimizer'])
        sched = getattr(torch.optim.lr_scheduler, config.get('lr_scheduler_type', ''), None)
        self.lr_scheduler = sched(self.optimizer, **config['lr_scheduler']) if sched else None
        self.lr_scheduler_freq = config.get('lr_scheduler_freq', 1)
        self.monitor, self.monitor_mode = config['trainer']['monitor'], config['trainer']['monitor_mode']
        assert self.monitor_mode in ('min', 'max')
        self.monitor_best = math.inf if self.monitor_mode == 'min' else -math.inf
        self.start_epoch = 1
        self.checkpoint_dir = os.path.join(config['trainer']['save_dir'], config['name'])
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        import json                      # base_trainer.py:50-51: the reference's test / evaluation tooling reads it beside the checkpoints
        with open(os.path.join(self.checkpoint_dir, 'config.json'), 'w') as f:
            json.dump(config, f, indent=4, sort_keys=False)
        self.train_logger = train_logger if train_logger is not None else ck.Logger()
        self.lr_history = []
        if resume:
            self.start_epoch, c = ck.resume(resume, model, self.optimizer, map_location='cpu')
            self.monitor_best = c['monitor_best']
            self.train_logger = c['logger']

    def _save(self, epoch, log, save_best=False):
        import os
        from . import checkpoint as ck
        path = ck.save_checkpoint(ck.checkpoint_name(self.checkpoint_dir, epoch, log['loss']), self.model, self.optimizer, epoch,
                                  self.config, self.monitor_best, self.train_logger)
        if save_best:
            best = os.path.join(self.checkpoint_dir, 'model_best.pth.tar')
            os.rename(path, best)
            path = best
        return path

    def train(self):
        for epoch in range(self.start_epoch, self.epochs + 1):
            result = self.train_epoch(epoch)
            log = {'epoch': epoch}
            log.update({k: v for k, v in result.items() if 'previews' not in k})
            self.train_logger.add_entry(log)
            if (self.monitor_mode == 'min' and log[self.monitor] < self.monitor_best) or \
                    (self.monitor_mode == 'max' and log[self.monitor] > self.monitor_best):
                self.monitor_best = log[self.monitor]
                self._save(epoch, log, save_best=True)
            if epoch % self.save_freq == 0:
                self._save(epoch, log)
            if self.lr_scheduler and epoch % self.lr_scheduler_freq == 0:
                self.lr_scheduler.step()
            self.lr_history.append(self.lr_scheduler.get_last_lr()[0] if self.lr_scheduler else self.optimizer.param_groups[0]['lr'])
        return self.train_logger


def select_evenly_spaced_elements(num_elements, sequence_length):
    """Preview indices (utils/training_utils.py:11-12)."""
    return [i * sequence_length // num_elements + sequence_length // (2 * num_elements) for i in range(num_elements)]


class SequenceTrainer:
    """The epoch loops of the reference's LSTMTrainer (`_train_epoch`, lstm_trainer.py:392-572, and `_valid_epoch`, :574-644) around
    `sequence_loss`, with the training metrics (model/metric.py) on the device — no TensorBoard, preview images, movies or gradient
    plots.  `train_epoch(epoch)` returns the reference's log entries ('loss', 'losses', 'metrics' and, with a validation loader,
    'val_loss', 'val_losses', 'val_metrics'), which is what `EpochTrainer(model, config, train_epoch=st.train_epoch)` monitors and
    stores in its checkpoints; `epoch_trainer()` builds that EpochTrainer and shares its optimizer.

    config keys, read as the reference reads them: config['trainer']['num_previews' | 'num_val_previews' | 'loss_composition' |
    'loss_weights'], config['loss'] ('type', 'config'), optional config['grad_loss'] / config['mse_loss'], config['metrics'],
    config['data_loader']['train']['every_x_rgb_frame'].  Not in the reference, optional: config['trainer']['freeze'] /
    config['trainer']['train_only'] — lists of patterns for `freeze` (partial training), applied to the model here.

    Mirrored semantics.  Every entry of 'losses' carries the aliasing factor (`loss_parts`); an epoch value is the sum over the
    batches / len(loader).  'metrics' = sum over the preview sequences and over ALL prediction keys of the metrics of (prediction of
    package 0, target of the last supervised key of package 0) / num_previews; the preview indices come from the number of BATCHES
    and index the DATASET (lstm_trainer.py:96, :490), items get a batch dimension, and the whole preview sequence is forwarded under
    no_grad in the mode the model is in (train mode in train_epoch: a BN model updates its running statistics, as the reference's).
    `valid_epoch` runs in eval mode under no_grad and leaves the model in eval mode.

    The batch loops do not synchronise with the host: loss parts go to rows of a device table, preview metrics to ONE
    metrics.batch_metrics call, and each epoch half reads back once at its end.  step_metrics=True adds the reference's never-reported
    `calculate_total_metrics` (:290-294: every prediction of every package against 'depth_<key>') as one batch_metrics call per step,
    averaged into 'step_metrics' / 'val_step_metrics'.  With a process group the float64 table of sums and batch counts is all-reduced
    at the end of each half, and the previews are chosen from the GLOBAL number of batches, so every rank logs the same values."""

    def __init__(self, config, model, data_loader, valid_data_loader=None, optimizer=None, reducer=None, process_group=None,
                 step_metrics=False):
        from . import metrics as M
        self.config, self.model, self.optimizer, self.reducer, self.group = config, model, optimizer, reducer, process_group
        self.data_loader, self.valid_data_loader = data_loader, valid_data_loader
        tr = config['trainer']
        apply_deterministic_config(config)
        self.frozen = apply_freeze_config(model, config)       # optional tr['freeze'] / tr['train_only'] (before epoch_trainer() builds the optimizer)
        self.num_previews, self.num_val_previews = tr['num_previews'], tr['num_val_previews']
        self.loss_composition, self.loss_weights = tr['loss_composition'], tr['loss_weights']
        self.loss_type = config['loss']['type']
        if self.loss_type not in LOSS_TYPES:
            raise KeyError("config['loss']['type'] = %r; known: %s" % (self.loss_type, ", ".join(LOSS_TYPES)))
        self.loss_params = config['loss'].get('config')
        self.grad_loss_weight = config['grad_loss'].get('weight', 1.0) if 'grad_loss' in config else None
        self.mse_loss = None
        if 'mse_loss' in config:
            self.mse_loss = {'weight': config['mse_loss'].get('weight', 1.0),
                             'downsampling_factor': config['mse_loss'].get('downsampling_factor', 0.5)}
        self.metrics = M.resolve_metrics(config['metrics'])
        self.every_x_rgb_frame = config['data_loader']['train']['every_x_rgb_frame']
        self.step_metrics = bool(step_metrics)
        self.loss_names = ['loss', 'L_si'] + (['L_grad'] if self.grad_loss_weight is not None else []) + (['L_mse'] if self.mse_loss else [])
        self.preview_indices = select_evenly_spaced_elements(self.num_previews, self._global_batches(data_loader))
        if valid_data_loader is not None:
            self.val_preview_indices = select_evenly_spaced_elements(self.num_val_previews, self._global_batches(valid_data_loader))

    def epoch_trainer(self, **kwargs):
        """EpochTrainer(model, config, train_epoch=self.train_epoch, reducer=self.reducer, **kwargs); this trainer steps ITS optimizer (the
        one its checkpoints store and a resume restores)."""
        et = EpochTrainer(self.model, self.config, self.train_epoch, reducer=self.reducer, **kwargs)
        self.optimizer = et.optimizer
        return et

    # ---- data parallel: sums over the ranks (one small float64 table per epoch half)
    def _world(self):
        import torch.distributed as dist
        return dist.get_world_size(self.group) if self.group is not None or (dist.is_available() and dist.is_initialized()) else 1

    def _global_batches(self, loader):
        n = len(loader)
        if self._world() > 1:
            import torch.distributed as dist
            t = torch.tensor([n], dtype=torch.int64)
            if dist.get_backend(self.group) == "nccl":
                t = t.to(self.model.gpu)
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
            n = int(t.item())
        return n

    def _all_reduce(self, table):
        if self._world() > 1:
            import torch.distributed as dist
            dist.all_reduce(table, op=dist.ReduceOp.SUM, group=self.group)
        return table

    # ---- one pass over a loader
    def _loss(self, sequence):
        return sequence_loss(self.model, sequence, self.loss_composition, self.loss_weights, loss_params=self.loss_params,
                             grad_loss_weight=self.grad_loss_weight, loss_type=self.loss_type, mse_loss=self.mse_loss, parts=True)

    def _step_metrics(self, sequence, predictions, acc):
        from . import metrics as M
        tab = M.batch_metrics([p for _, _, p in predictions], [sequence[l]['depth_' + key] for l, key, _ in predictions], self.metrics)
        acc[:-1] += tab.sum(0)
        acc[-1] += tab.shape[0]

    def _previews(self, dataset, indices):
        """-> float64 [len(metrics)] on the device: the preview metrics summed over sequences and keys (not yet / num_previews)."""
        from . import metrics as M
        preds, targets = [], []
        K = self.model.every_x_rgb_frame
        with torch.no_grad():
            for idx in indices:
                sequence = dataset[idx]
                prev_super, prev_lstm, first = None, empty_states_lstm(K), True
                for item in sequence:
                    # [C, H, W] items get the batch dimension (lstm_trainer.py:497-500: every key but an already batched 'depth_image')
                    item = {k: (v.unsqueeze(0) if torch.is_tensor(v) and (k != 'depth_image' or v.dim() < 4) else v) for k, v in item.items()}
                    out, supers, lstms = self.model(item, prev_super, prev_lstm)
                    if first:
                        target = None
                        for key in out:
                            if not self.loss_composition or key in self.loss_composition:
                                target = item['depth_' + key]          # `new_target`: the last supervised key iterated (:282, :377)
                        if target is None:
                            raise ValueError("preview %d: package 0 has no supervised prediction (loss_composition %r, predictions %r)"
                                             % (idx, self.loss_composition, list(out)))
                        for key, value in out.items():
                            preds.append(value.detach())
                            targets.append(target)
                        first = False
                    prev_super, prev_lstm = supers['image'], lstms
            if not preds:
                return torch.zeros(len(self.metrics), device=self.model.gpu, dtype=torch.float64)
            return M.batch_metrics(preds, targets, self.metrics).sum(0)

    def _run(self, loader, dataset_indices, n_previews, train):
        """-> (losses dict, metrics list, step metrics list or None); one device -> host copy."""
        dev = self.model.gpu
        nl, nm = len(self.loss_names), len(self.metrics)
        n_batches = len(loader)
        rows = torch.zeros((max(n_batches, 1), nl), device=dev, dtype=torch.float64)
        step_acc = torch.zeros(nm + 1, device=dev, dtype=torch.float64) if self.step_metrics else None
        for i, sequence in enumerate(loader):
            if train:
                if self.reducer is not None:
                    self.reducer.zero()
                else:
                    self.optimizer.zero_grad()
            total, _, parts = self._loss(sequence)
            if train:
                total.backward()
                if self.reducer is not None:
                    self.reducer.all_reduce()
                    self.reducer.wait()
                self.optimizer.step()
            if i >= rows.shape[0]:
                raise RuntimeError("the loader yielded more batches than len(loader) = %d" % n_batches)
            rows[i].copy_(torch.stack([parts[k].reshape(()) for k in self.loss_names]))
            if step_acc is not None:
                with torch.no_grad():
                    self._step_metrics(sequence, parts['predictions'], step_acc)
        previews = self._previews(loader.dataset, dataset_indices)
        # [loss sums | batches | preview metric sums | step metric sums, pairs]: the ranks' tables add up
        table = torch.cat([rows.sum(0), torch.full((1,), float(n_batches), device=dev, dtype=torch.float64), previews]
                          + ([step_acc] if step_acc is not None else []))
        world = self._world()
        host = self._all_reduce(table).cpu().tolist()
        losses = {k: host[j] / host[nl] for j, k in enumerate(self.loss_names)}
        metrics = [v / world / n_previews for v in host[nl + 1:nl + 1 + nm]]          # (every rank forwards the same previews)
        steps = [v / host[-1] for v in host[nl + 1 + nm:-1]] if step_acc is not None else None
        return losses, metrics, steps

    def train_epoch(self, epoch):
        if self.optimizer is None:
            raise RuntimeError("SequenceTrainer: no optimizer (pass one, or build the EpochTrainer with epoch_trainer())")
        self.model.train()
        losses, metrics, steps = self._run(self.data_loader, self.preview_indices, self.num_previews, True)
        log = {'loss': losses['loss'], 'losses': losses, 'metrics': metrics}
        if steps is not None:
            log['step_metrics'] = steps
        if self.valid_data_loader is not None:
            log.update(self.valid_epoch(epoch))
        return log

    def valid_epoch(self, epoch=0):
        self.model.eval()
        with torch.no_grad():
            losses, metrics, steps = self._run(self.valid_data_loader, self.val_preview_indices, self.num_val_previews, False)
        log = {'val_loss': losses['loss'], 'val_losses': losses, 'val_metrics': metrics}
        if steps is not None:
            log['val_step_metrics'] = steps
        return log
