"""The reference's training and validation schedules, written once: train_epoch() and validate() over a *group* of R models
(model.Replicas as it stands; a single RNN / DiffDelRNN through model._Single, R = 1), and the segment loop of predict().

The two schedules (code/model.py:90-216 for RNN, :426-616 for DiffDelRNN) are RNN_SCHEDULE and DIFFDEL_SCHEDULE below; nothing else
in the package states a warm-up or window length.  The loops touch a group through
    models, name, device, schedule          the R modules, the class name for messages, where batches go, one of the two below
    reset(Bper)                             every model's initialize_hidden for Bper streams each
    stepper(train) -> step                  step(x, d_traj or None, warmup) -> (pred, pre_d or None), stateful, on (R*Bper, 1, T)
                                            replica-major tensors; in training form (graph nodes) or inference form
    detach_hidden(), zero_grad()
    grouped_loss(loss_fcn)                  (pred, target) -> [R] losses in one go, or None: loss_fcn is applied per replica
and never touch a device themselves, so tests/test_epoch_loops_cpu.py drives them with a stub group in plain torch."""
from collections import namedtuple

import numpy as np
import torch

# warmup(dataset) -> samples that only aggregate state;  window: samples per TBPTT window / validation piece;  delays: the batches
# carry a delay trajectory;  train_windows(n, window) -> windows in the n samples after the warm-up;  val_pieces(n, window) -> pieces
# whose mean is a batch's validation loss, or None: everything after the warm-up is scored as one piece, with no division
Schedule = namedtuple("Schedule", "warmup window delays train_windows val_pieces")


def _diffdel_warmup(dataset):
    """Warm-up length of a DiffDel dataset in samples: nextpow2(int(max_delay * fs)), max_delay in seconds from
    `delay_analyzer.max_delay` (the reference's dataset) or `max_delay` (SegmentFeeder)."""
    from .utilities import nextpow2
    max_delay = dataset.delay_analyzer.max_delay if hasattr(dataset, "delay_analyzer") else dataset.max_delay
    return nextpow2(int(max_delay * dataset.fs))


RNN_SCHEDULE = Schedule(warmup=lambda dataset: 2**10, window=2**10, delays=False,
                        train_windows=lambda n, window: n // window, val_pieces=None)
DIFFDEL_SCHEDULE = Schedule(warmup=_diffdel_warmup, window=2**11, delays=True,
                            train_windows=lambda n, window: int(np.ceil(n // window)),
                            val_pieces=lambda n, window: int(np.ceil(n / window)))


# ---- what train_epoch / validate do to a batch before their loop
def _audio_channel(input, target, device):
    """(input, target) (B,C,T) -> channel 0 of both on `device`: only the audio channel counts for training and for the loss."""
    if input.shape[1] > 1:
        input, target = input[:, :1, :], target[:, :1, :]
    return input.to(device), target.to(device)


def _delay_samples(extra, fs, who):
    """The delay trajectory (B,1,T) in samples -- the fp32 product d_seconds * fs, as the reference forms it -- from the third item
    of a batch: the reference's meta dict with 'delay_trajectory' (B,T) in seconds, or SegmentFeeder.batches' d_seconds (B,C,T)."""
    if isinstance(extra, dict):
        d_traj = extra["delay_trajectory"].float()
        return d_traj.unsqueeze(1) * fs
    if extra is not None:
        return extra[:, :1, :].float() * fs
    raise RuntimeError(f"{who}: the batch carries no delay trajectory")


def _is_batch(b):
    return isinstance(b, (tuple, list)) and len(b) >= 2 and torch.is_tensor(b[0])


def _per_replica(arg, R, what, who):
    """-> (list of R, shared): `arg` is a list / tuple of R loaders (none of whose items is itself a batch), or ONE loader
    (which may itself be a list of batches) shared by all replicas."""
    if isinstance(arg, (list, tuple)) and arg and not any(_is_batch(b) for b in arg):
        if len(arg) != R:
            raise ValueError(f"{who}: {len(arg)} {what} for {R} replicas")
        return list(arg), False
    return [arg] * R, True


def _lockstep(loaders, shared):
    """The R batches of every iteration: the shared loader's batch R times, or one from each loader (ends with the shortest)."""
    return ((b,) * len(loaders) for b in loaders[0]) if shared else zip(*loaders)


def _plan(group, loaders, dataset, who):
    """-> (the warm-up length, prepare(r, input, target, extra) -> replica r's batch as its model's own loop prepares it:
    (input, target[, d_traj in samples]), channel 0, on the group's device).  With delays every replica has a dataset (default its
    loader's .dataset) for `fs` and the warm-up length, which must be one for all."""
    sch, R, device = group.schedule, len(group.models), group.device
    if not sch.delays:
        return sch.warmup(None), lambda r, input, target, extra: _audio_channel(input, target, device)
    datasets = ([ld.dataset for ld in loaders] if dataset is None else
                list(dataset) if isinstance(dataset, (list, tuple)) else [dataset] * R)
    if len(datasets) != R:
        raise ValueError(f"{who}: {len(datasets)} datasets for {R} replicas")
    fss = [ds.fs for ds in datasets]
    inits = [sch.warmup(ds) for ds in datasets]
    if len(set(inits)) != 1:
        raise ValueError(f"{who}: the datasets give different warm-up lengths {inits}; one is needed")

    def prepare(r, input, target, extra):
        return _audio_channel(input, target, device) + (_delay_samples(extra, fss[r], who).to(device),)
    return inits[0], prepare


def _gather(batches, prepare, who):
    """The R batches of one iteration, each prepared, -> (stacked replica-major, the R prepared batches as they were before
    stacking).  All R must have one shape: ValueError naming both shapes otherwise, before anything is launched for the
    iteration.  R = 1: the prepared batch itself, no copy."""
    R = len(batches)
    for r, batch in enumerate(batches):
        for a, b in zip(batches[0][:2], batch[:2]):
            if a.shape != b.shape:
                raise ValueError(f"{who}: the batch of replica {r} has shape {tuple(b.shape)}, that of replica 0 "
                                 f"{tuple(a.shape)}; all replicas need batches of one shape")
    per = [prepare(r, b) for r, b in enumerate(batches)]
    if R == 1:
        stacked = list(per[0])
    elif all(b is batches[0] for b in batches):
        stacked = [t.repeat(R, 1, 1) for t in per[0]]
    else:
        stacked = [torch.cat(ts, dim=0) for ts in zip(*per)]
    return stacked, per


def _rows(t, r, R):
    """Replica r's streams of a replica-major tensor (the tensor itself for R = 1)."""
    n = t.shape[0] // R
    return t if R == 1 else t[r * n:(r + 1) * n]


def _cut(input, d_traj, sl):
    """Samples `sl` of the input and of the delay trajectory (None where there is none)."""
    return input[:, :, sl], None if d_traj is None else d_traj[:, :, sl]


def train_epoch(group, dataloaders, loss_fcn, optimizers, dataset=None, losses_hook=None):
    """One epoch of truncated back-propagation through time for every model of the group, in lock step; -> the list of R epoch
    losses (mean over batches of the mean window loss).  Per batch: reset, the warm-up forward with grad enabled and NOT detached
    (window 1's backward reaches through it), zero_grad, then per whole window forward, loss, backward (of the sum of the R losses:
    they share no node, so each model receives its own gradient; one model without a grouped loss: of its loss as it is -- a stack
    and a sum of one cost 1 % of a 1024-sample window), every optimizer's step(), detach_hidden, zero_grad, and ONE host
    synchronisation for the R loss values.  Arguments: model.Replicas.train_epoch."""
    who = group.name + ".train_epoch"
    sch, R = group.schedule, len(group.models)
    loaders, shared = _per_replica(dataloaders, R, "loaders", who)
    opts = list(optimizers) if isinstance(optimizers, (list, tuple)) else [optimizers]
    for m in group.models:
        m._check_trainable(who)
        for p in m.parameters():
            p.requires_grad_(True)
        m.train()
    init, prepare = _plan(group, loaders, dataset, who)
    many = group.grouped_loss(loss_fcn)
    step = group.stepper(train=True)

    num_batches = 0             # counted, so that a generator (SegmentFeeder.batches) serves as well as a DataLoader
    epoch_loss = [0] * R
    for batches in _lockstep(loaders, shared):
        stacked, _ = _gather(batches, lambda r, b: prepare(r, b[0], b[1], b[2] if sch.delays else None), who)
        input, target = stacked[0], stacked[1]
        d_traj = stacked[2] if sch.delays else None

        num_minibatches = sch.train_windows(input.shape[-1] - init, sch.window)
        group.reset(input.shape[0] // R)
        step(*_cut(input, d_traj, slice(0, init)), True)                    # graph nodes: window 1's backward reaches them
        group.zero_grad()

        minibatch_loss = [0] * R
        sample_offset = init
        for _ in range(num_minibatches):
            sl = slice(sample_offset, sample_offset + sch.window)
            pred_mini, _ = step(*_cut(input, d_traj, sl), False)
            target_mini = target[:, :, sl]
            if many is not None:
                losses = many(pred_mini, target_mini)
            elif R > 1:
                losses = torch.stack([loss_fcn(_rows(pred_mini, r, R), _rows(target_mini, r, R)).reshape(()) for r in range(R)])
            else:
                losses = loss_fcn(pred_mini, target_mini)                   # one model: backward() on its loss as it is
            (losses.sum() if losses.dim() else losses).backward()
            for opt in opts:
                opt.step()
            group.detach_hidden()
            group.zero_grad()
            values = losses.tolist() if losses.dim() else [losses.item()]      # one host synchronisation for the R losses
            if losses_hook is not None:
                losses_hook(values)
            minibatch_loss = [a + v for a, v in zip(minibatch_loss, values)]
            sample_offset += sch.window
        minibatch_loss = [a / num_minibatches for a in minibatch_loss]      # ZeroDivisionError when no whole window follows the
        epoch_loss = [a + b for a, b in zip(epoch_loss, minibatch_loss)]    # warm-up (RNN: T < 2048), as in the reference
        num_batches += 1
    return [a / num_batches for a in epoch_loss]


def _host_rows(rows):
    """The losses of one batch, rows [pieces][R], as Python floats -- the values `.item()` gives -- brought over in ONE .tolist()
    of a [pieces, R] tensor wherever they are several tensors of one kind on one device."""
    if rows and all(torch.is_tensor(r) for r in rows):
        return torch.stack(rows).tolist()
    flat = [v for r in rows for v in r]
    if len(flat) > 1 and all(torch.is_tensor(v) and v.dtype == flat[0].dtype and v.device == flat[0].device for v in flat):
        return torch.stack([v.reshape(()) for v in flat]).view(len(rows), -1).tolist()
    return [[v.item() if hasattr(v, "item") else float(v) for v in r] for r in rows]


@torch.no_grad()
def validate(group, dataloaders, loss_fcn, store_examples=True):
    """The validation loss of every model of the group, in lock step; -> the list of R (mean loss over batches, examples).  Per
    batch: reset, the state aggregated on the warm-up's REAL samples, the rest predicted in ONE forward and scored -- as one piece,
    or on `window`-sample pieces whose mean is the batch's loss (the reference forwards those one by one; chunked == one-shot bit
    for bit).  A loss without a grouped form sees, for every replica, tensors laid out as the single model's loop lays them out:
    with pieces, slices of a whole-length fp32 buffer filled from the warm-up on; else a fresh contiguous prediction; and the
    replica's own target sliced after the warm-up -- so that a torch reduction takes the same path for every R.  The losses of a
    batch reach the host together and are added in Python in piece order.  Arguments: model.Replicas.validate."""
    who = group.name + ".validate"
    sch, R, device = group.schedule, len(group.models), group.device
    loaders, shared = _per_replica(dataloaders, R, "loaders", who)
    counts = [len(ld) for ld in loaders]
    if len(set(counts)) != 1:
        raise ValueError(f"{who}: the loaders have different lengths {counts}; every replica needs as many batches")
    for m in group.models:
        m.eval()
    init, prepare = _plan(group, loaders, None, who)
    many = group.grouped_loss(loss_fcn)
    step = group.stepper(train=False)           # once per call, not once per batch

    def unpack(r, batch):
        input, target, meta = batch
        return prepare(r, input, target, meta)

    val_loss = [0] * R
    examples = [[] for _ in range(R)]
    for batches in _lockstep(loaders, shared):
        stacked, per = _gather(batches, unpack, who)
        input, target = stacked[0], stacked[1]
        d_traj = stacked[2] if sch.delays else None
        T = input.shape[-1]
        num_minibatches = None if sch.val_pieces is None else sch.val_pieces(T - init, sch.window)
        group.reset(input.shape[0] // R)
        step(*_cut(input, d_traj, slice(0, init)), True)
        if num_minibatches is None or num_minibatches > 0:
            pred, pre_d = step(*_cut(input, d_traj, slice(init, None)), False)
        else:
            pred = pre_d = torch.empty(input.shape[0], 1, max(T - init, 0), device=device, dtype=torch.float32)
        pieces = ([slice(None)] if num_minibatches is None else
                  [slice(k * sch.window, (k + 1) * sch.window) for k in range(num_minibatches)])
        input, target = input[:, :, init:], target[:, :, init:]
        if many is not None:
            rows = [many(pred[:, :, sl], target[:, :, sl]) for sl in pieces]
        else:
            rows = [[] for _ in pieces]
            for r in range(R):
                own_p, own_t = _rows(pred, r, R), per[r][1]
                if num_minibatches is not None:
                    whole = torch.empty(own_t.shape, device=device, dtype=torch.float32)
                    whole[:, :, init:] = own_p
                    own_p = whole[:, :, init:]
                elif R > 1:
                    own_p = own_p.clone()
                own_t = own_t[:, :, init:]
                for k, sl in enumerate(pieces):
                    rows[k].append(loss_fcn(own_p[:, :, sl], own_t[:, :, sl]))
        batch_loss = [0] * R
        for values in _host_rows(rows):                             # in piece order
            batch_loss = [a + v for a, v in zip(batch_loss, values)]
        if num_minibatches is not None:
            batch_loss = [a / num_minibatches for a in batch_loss]  # ZeroDivisionError for T <= the warm-up, as in the reference
        val_loss = [a + b for a, b in zip(val_loss, batch_loss)]
        if store_examples:
            n = input.shape[0] // R
            for r in range(R):
                ex = {"input": input[r * n, 0, :], "target": target[r * n, 0, :], "prediction": pred[r * n, 0, :]}
                if sch.delays:
                    ex["prediction_pre_d"] = pre_d[r * n, 0, :]
                examples[r].append(ex)
    return [(v / c, ex) for v, c, ex in zip(val_loss, counts, examples)]


def in_segments(run, input, segment_length, outputs=1):
    """predict()'s loop: run(slice) -> a tuple of `outputs` tensors (.., .., length of the slice), stateful, over the whole of
    input (N, C, T) at once (`segment_length` None) or over `segment_length`-sample slices in order, written into preallocated
    fp32 outputs of input's shape (code/model.py:218-246, :618-653); -> the tuple of outputs."""
    if segment_length is None:
        return tuple(run(slice(None)))
    outs = tuple(torch.empty(input.shape, device=input.device, dtype=torch.float32) for _ in range(outputs))
    for i in range(int(np.ceil(input.shape[-1] / segment_length))):
        sl = slice(i * segment_length, (i + 1) * segment_length)
        for o, v in zip(outs, run(sl)):
            o[:, :, sl] = v
    return outs
