#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Training CLI, drop-in for the reference's ``wavenet_vocoder/bin/train.py``.

Same command line (every flag of train.py:339-393, ``strtobool`` booleans, ``--resume ""``), same
outputs (``expdir/model.conf``, ``checkpoint-%d.pkl`` = {"model","optimizer","iterations"},
``checkpoint-final.pkl`` = {"model"}; train.py:315-332,429,564-568) and the same log lines
("(iter:%d) average loss = %.6f (%.3f sec / batch)", train.py:547), so ``egs/*/run.sh`` stage 4
runs unchanged.  What differs is how a step is executed:

  * forward / cross-entropy / backward run in the HIP kernels (``WaveNet.loss_and_backward``) and
    Adam is one fused launch over the flat parameter buffer (``FusedAdam``);
  * ``--n_gpus N`` starts ONE PROCESS PER GPU (torch.distributed over RCCL) instead of
    ``nn.DataParallel`` (train.py:449-454): every rank takes its 1/N slice of each minibatch along
    dim 0 -- exactly the chunks DataParallel scatters -- computes its own loss, and the flat
    gradient buffer is all-reduced in buckets on a side stream while backward is still running;
  * the wav / feature / stats readers fall back to scipy / .npz when soundfile / h5py are absent.
"""
import argparse
import contextlib
import logging
import os
import re
import sys
import time

import numpy as np
import torch

from pytorchwavenetvocoder_amd.adapters import AdapterAdam, LowRankAdapters
from pytorchwavenetvocoder_amd.nets import WaveNet, encode_mu_law, initialize
from pytorchwavenetvocoder_amd.utils import background, extend_time, find_files, make_feat_transform, read_hdf5, read_txt


def strtobool(v):
    """distutils.util.strtobool (the reference's flag parser, train.py:13,366-369)."""
    v = str(v).lower()
    if v in ("y", "yes", "t", "true", "on", "1"):
        return 1
    if v in ("n", "no", "f", "false", "off", "0"):
        return 0
    raise ValueError("invalid truth value %r" % (v,))


def read_wav(path):
    """float32 waveform in [-1, 1] and sampling rate (soundfile when available, else scipy)."""
    try:
        import soundfile as sf
        return sf.read(path, dtype=np.float32)
    except ImportError:
        from scipy.io import wavfile
        fs, x = wavfile.read(path)
        if x.dtype == np.int16:
            x = x.astype(np.float32) / 32768.0
        elif x.dtype == np.int32:
            x = x.astype(np.float32) / 2147483648.0
        else:
            x = x.astype(np.float32)
        return x, fs


def validate_length(x, y, upsampling_factor=None):
    """Trim waveform ``x`` and features ``y`` to consistent lengths.  A deliberate RESTATEMENT of reference train.py:35-64
    (13 lines of required index behaviour; pinned against the reference by tests/golden/slicer.npz)."""
    if upsampling_factor is None:
        n = min(x.shape[0], y.shape[0])
        x, y = x[:n], y[:n]
        assert len(x) == len(y)
    else:
        if x.shape[0] > y.shape[0] * upsampling_factor:
            x = x[:y.shape[0] * upsampling_factor]
        if x.shape[0] < y.shape[0] * upsampling_factor:
            mod_y = y.shape[0] * upsampling_factor - x.shape[0]
            mod_y_frame = mod_y // upsampling_factor + 1
            y = y[:-mod_y_frame]
            x = x[:y.shape[0] * upsampling_factor]
        assert len(x) == len(y) * upsampling_factor
    return x, y


def _to_batch(xs, hs, ts, device, ys=None):
    tensors = [torch.stack(xs), torch.stack(hs), torch.stack(ts)] + ([torch.stack(ys)] if ys else [])
    if device is not None:
        if torch.device(device).type == "cuda":  # pinned staging: the copies overlap the step that is running
            tensors = [v.pin_memory() for v in tensors]
        tensors = [v.to(device, non_blocking=True) for v in tensors]
    if ys:
        return (tensors[0], tensors[1]), tensors[2], tensors[3]
    return (tensors[0], tensors[1]), tensors[2]


def _shard_range(batch_size, shard):
    """Window indices [lo, hi) of a minibatch owned by rank ``shard[0]`` of ``shard[1]`` -- the chunks
    ``nn.DataParallel`` scatters (reference train.py:449-454)."""
    if shard is None:
        return 0, batch_size
    rank, world = shard
    if batch_size < world:
        raise ValueError("batch_size (%d) must be >= the number of ranks (%d): every rank needs a window of each "
                         "minibatch, or it would never reach the gradient all-reduce" % (batch_size, world))
    # as even as possible, never empty: the first batch_size % world ranks own one window more
    per, extra = divmod(batch_size, world)
    lo = rank * per + min(rank, extra)
    return lo, lo + per + (1 if rank < extra else 0)


def slicer_workers():
    """Worker threads of the window slicer: ``WN_SLICER_WORKERS`` (0 = everything in the producer thread, as the reference does),
    default min(4, CPUs - 1).  numpy / zlib / file reads / torch.stack release the GIL, so threads do run in parallel here."""
    v = os.environ.get("WN_SLICER_WORKERS")
    if v is not None:
        return max(0, int(v))
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(0, min(4, n - 1))


class _Done(object):
    """A finished 'future' (the inline path of the slicer: same code, no pool)."""

    def __init__(self, value):
        self.value = value

    def result(self):
        return self.value


def _load_utterance(wavfile, featfile, feature_type, upsampling_factor, use_upsampling_layer, use_speaker_code,
                    wav_transform, feat_transform, pre):
    """one utterance from its two files, trimmed to consistent lengths (train.py:202-212): (x, h, None, None), or with ``pre``
    (x, h, transformed x, transformed h) -- the transforms applied once per utterance (``transforms_elementwise``)"""
    x, _fs = read_wav(wavfile)
    h = read_hdf5(featfile, "/" + feature_type)
    if not use_upsampling_layer:
        h = extend_time(h, upsampling_factor)
    if use_speaker_code:
        sc = read_hdf5(featfile, "/speaker_code")
        h = np.concatenate([h, np.tile(sc, [h.shape[0], 1])], axis=1)
    x, h = validate_length(x, h, upsampling_factor if use_upsampling_layer else None)
    if not pre:
        return x, h, None, None
    # the buffers' dtypes (float32 waveform; features promoted with float32) are what the per-window transforms would see
    xf = np.asarray(x, dtype=np.float32)
    hf = np.asarray(h, dtype=np.result_type(np.float32, np.asarray(h).dtype))
    return xf, hf, (wav_transform(xf) if wav_transform is not None else xf), (feat_transform(hf) if feat_transform is not None else hf)


def _prep_window(x_, h_, xt_, ht_, wav_transform, feat_transform):
    """one window: (tokens, features, un-quantised waveform); xt_ / ht_: the slices of the already transformed utterances"""
    raw = torch.from_numpy(np.asarray(x_, dtype=np.float32))
    if xt_ is not None:
        x_, h_ = xt_, ht_
    else:
        if wav_transform is not None:
            x_ = wav_transform(x_)
        if feat_transform is not None:
            h_ = feat_transform(h_)
    return torch.from_numpy(np.asarray(x_)).long(), torch.from_numpy(np.asarray(h_)).float(), raw


def _whole_utterance(x, h, xt, ht, upsampling_factor, use_upsampling_layer):
    """an utterance as ONE window (the utterance modes, train.py:288-291): with the upsampling layer a whole number of frames"""
    if use_upsampling_layer:
        h = h[:-1]
        x = x[:-upsampling_factor + 1]
        if xt is not None:
            ht = ht[:-1]
            xt = xt[:-upsampling_factor + 1]
    return x, h, xt, ht


def _window_rows(windows, use_upsampling_layer):
    """prepared windows -> the rows of a minibatch: inputs x[:-1], features (D, frames), targets x[1:] and waveform[1:]"""
    xs, hs, ts, ys = [], [], [], []
    for x_, h_, raw in windows:
        hs.append(h_.transpose(0, 1) if use_upsampling_layer else h_[:-1].transpose(0, 1))
        xs.append(x_[:-1])
        ts.append(x_[1:])
        ys.append(raw[1:])
    return xs, hs, ts, ys


def _pad_rows(xs, hs, ts, ys, n_quantize):
    """rows of unequal length padded to the longest: tokens and targets with n_quantize // 2, the waveform with 0, the features
    by repeating the last frame; + the valid positions of every row (CPU int64)"""
    lengths = torch.tensor([int(v.numel()) for v in xs], dtype=torch.int64)
    T = int(lengths.max())
    F = max(int(v.size(1)) for v in hs)
    fill = int(n_quantize) // 2
    xs = [torch.nn.functional.pad(v, (0, T - v.numel()), value=fill) for v in xs]
    ts = [torch.nn.functional.pad(v, (0, T - v.numel()), value=fill) for v in ts]
    ys = [torch.nn.functional.pad(v, (0, T - v.numel()), value=0.0) for v in ys]
    hs = [torch.cat([v, v[:, -1:].expand(-1, F - v.size(1))], dim=1) if v.size(1) < F else v for v in hs]
    return xs, hs, ts, ys, lengths


@background(max_prefetch=16)
def train_generator(wav_list, feat_list, receptive_field,
                    batch_length=None,
                    batch_size=1,
                    feature_type="world",
                    wav_transform=None,
                    feat_transform=None,
                    shuffle=True,
                    upsampling_factor=80,
                    use_upsampling_layer=True,
                    use_speaker_code=False,
                    device="auto",
                    shard=None,
                    with_wave=False,
                    workers=None,
                    transforms_elementwise=False,
                    pad_utterances=False,
                    n_quantize=256):
    """Minibatch generator with the reference's four batching modes (train.py:67-312).

    Yields ``((batch_x, batch_h), batch_t)``: x/t int64 (B, T) with t the next sample of x, h float
    (B, D, T) -- or (B, D, T / upsampling_factor) with the upsampling layer.  Windows hold
    ``receptive_field + batch_length`` samples and advance by ``batch_length`` (the first
    receptive_field outputs of every window carry no loss, train.py:535).

    ``shard=(rank, world)``: yield only this rank's windows of every minibatch (same minibatch
    composition as the unsharded generator; the mu-law / scaling work of the other ranks' windows is
    skipped instead of being done ``world`` times).
    ``with_wave=True`` (mixture-of-logistics head): additionally yields ``batch_y`` float (B, T), the waveform
    value of the next sample at every position (the un-quantised counterpart of ``batch_t``).

    ``pad_utterances=True`` (NOT a reference mode; only with ``batch_length=None`` and ``batch_size > 1``, where the reference
    falls back to a batch size of 1 because its loss has no mask): ``batch_size`` consecutive utterances of the list are
    padded to the longest of them and yielded as ONE minibatch, followed by ``lengths`` and ``all_lengths`` (CPU int64
    tensors): the valid positions of the rows yielded, for ``loss_and_backward(lengths=)``, and of all ``batch_size``
    rows of the minibatch.  Tokens and targets pad with ``n_quantize // 2``, features by repeating the utterance's last
    frame, the waveform of ``with_wave`` with 0; with the upsampling layer an utterance is a whole number of frames, so T
    stays a multiple of ``upsampling_factor``.  ``shard=(rank, world)``: a rank takes its ``_shard_range`` rows of every
    minibatch and pads to ITS OWN longest utterance (ranks may run different T); every rank reads every utterance in this
    mode already, so ``all_lengths`` -- and with it the global count of loss positions -- needs no communication.  A
    group left incomplete at the end of a walk of the list is dropped, like a partly filled minibatch of the windowed modes.

    ``workers`` (default ``slicer_workers()``): the reference's generator is ONE numpy thread behind a queue that is in effect one
    deep (train.py:67, utils.py:216) -- at 8.7 ms per minibatch on an MI355X that thread (file reads 3 ms, mu-law 1.5 ms, scaler,
    stacking, pinning: 6.5 ms per minibatch of 8 windows) is as slow as the step.  Here the SEQUENTIAL part -- the order of the
    utterances, the running buffers, where each window is cut: a few slices per window -- stays in the producer thread, and the
    work hangs off it as jobs of a thread pool whose results are consumed in submission order: (1) read + validate utterance
    i + 1 ... i + 8 while utterance i is being cut, (2) mu-law / scaler / tensor conversion per window, (3) stack + pinned
    staging + H2D per minibatch.  Same functions on the same slices in the same order: the minibatches are bit-identical to the
    single-thread generator's (tests/test_train_cli.py: the reference generator's golden minibatches, with and without workers).

    ``transforms_elementwise=True`` (what the CLI passes: its mu-law and scaler are per-sample / per-frame maps): the two
    transforms are applied ONCE per utterance when it is read instead of once per window on the buffer slices -- windows overlap
    by the receptive field (15 % of the samples at the benchmark's geometry), and the work moves into the coarse per-utterance
    read jobs.  Same values bit for bit (a per-element map commutes with slicing; same dtypes: golden test)."""
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    if device == "auto":
        device = torch.device("cuda") if torch.cuda.is_available() else None
    if shuffle:
        n_files = len(wav_list)
        idx = np.random.permutation(n_files)
        wav_list = [wav_list[i] for i in idx]
        feat_list = [feat_list[i] for i in idx]
    if batch_length is not None and use_upsampling_layer:
        batch_mod = (receptive_field + batch_length) % upsampling_factor
        logging.warning("batch length is decreased due to upsampling (%d -> %d)" % (
            batch_length, batch_length - batch_mod))
        batch_length -= batch_mod
    padded = bool(pad_utterances) and batch_length is None and batch_size > 1
    if batch_length is None and batch_size > 1 and not padded:
        logging.warning("in utterance batch mode, batchsize will be 1.")
    pre = bool(transforms_elementwise)
    n_workers = slicer_workers() if workers is None else max(0, int(workers))
    pool = ThreadPoolExecutor(max_workers=n_workers, thread_name_prefix="wn_slicer") if n_workers > 0 else None

    def submit(fn, *a):
        return pool.submit(fn, *a) if pool is not None else _Done(fn(*a))

    def load(wavfile, featfile):
        return _load_utterance(wavfile, featfile, feature_type, upsampling_factor, use_upsampling_layer, use_speaker_code,
                               wav_transform, feat_transform, pre)

    def prep(x_, h_, xt_=None, ht_=None):
        return _prep_window(x_, h_, xt_, ht_, wav_transform, feat_transform)

    def assemble(window_jobs):
        """one minibatch from its windows' jobs (submitted before this one: the pool's queue is FIFO, so they are running or done)"""
        xs, hs, ts, ys = _window_rows([job.result() for job in window_jobs], use_upsampling_layer)
        return _to_batch(xs, hs, ts, device, ys if with_wave else None)

    def assemble_padded(window_jobs, all_lengths, lo):
        """one minibatch of whole utterances (this rank's rows [lo, lo + len(window_jobs)) of it), padded to the longest row"""
        xs, hs, ts, ys = _window_rows([job.result() for job in window_jobs], use_upsampling_layer)
        xs, hs, ts, ys, lengths = _pad_rows(xs, hs, ts, ys, n_quantize)
        assert lengths.tolist() == all_lengths[lo:lo + len(xs)]
        return _to_batch(xs, hs, ts, device, ys if with_wave else None) + (lengths, torch.tensor(all_lengths, dtype=torch.int64))

    def utterances():
        """(x, h) of the utterances in list order, epoch after epoch, ``None`` between two epochs (the reference's generator starts
        every walk of the list with an empty minibatch, train.py:196-200); the list is reshuffled where the reference reshuffles
        it (when it has been walked: the same sequence of np.random calls); up to ``ahead`` utterances are being read in front of
        the consumer, across the epoch boundary too"""
        nonlocal wav_list, feat_list
        ahead = 2 * n_workers if pool is not None else 0
        pending = deque()
        while True:
            for pair in zip(wav_list, feat_list):
                pending.append(submit(load, *pair))
                while len(pending) > ahead:
                    yield pending.popleft().result()
            pending.append(_Done(None))
            if shuffle:
                idx = np.random.permutation(n_files)
                wav_list = [wav_list[i] for i in idx]
                feat_list = [feat_list[i] for i in idx]

    # window sharding only exists in the windowed modes; utterance batches (batch_length None, effective batch size 1)
    # are dealt round-robin by utterance below, so a batch_size below the world size is fine there
    my_lo, my_hi = _shard_range(batch_size, shard) if (batch_length is not None or padded) else (0, batch_size)
    group_lengths = []                  # padded utterance batches: valid positions of every row of the minibatch being filled
    ready = deque()                     # minibatch jobs in the order they will be yielded
    max_ready = 2 * n_workers + 1 if pool is not None else 1
    x_buffer = h_buffer = xt_buffer = ht_buffer = None
    window_jobs = []
    n_in_batch = 0
    n_seen = 0                          # utterances of the current epoch (utterance mode: round-robin over ranks)
    try:
        for utt in utterances():
            if utt is None:             # a new walk of the list: the reference drops a partly filled minibatch here (the buffers stay)
                window_jobs = []
                group_lengths = []
                n_in_batch = 0
                n_seen = 0
                continue
            x, h, xt, ht = utt
            if batch_length is not None:
                # windowed minibatches over a running buffer of concatenated utterances
                if x_buffer is None:
                    x_buffer = np.empty((0), dtype=np.float32)
                    h_buffer = np.empty((0, h.shape[1]), dtype=np.float32)
                    if pre:
                        xt_buffer = np.empty((0), dtype=np.asarray(xt).dtype)
                        ht_buffer = np.empty((0, h.shape[1]), dtype=np.asarray(ht).dtype)
                x_buffer = np.concatenate([x_buffer, x], axis=0)
                h_buffer = np.concatenate([h_buffer, h], axis=0)
                if pre:
                    xt_buffer = np.concatenate([xt_buffer, xt], axis=0)
                    ht_buffer = np.concatenate([ht_buffer, ht], axis=0)
                if use_upsampling_layer:
                    h_bs = (receptive_field + batch_length) // upsampling_factor   # frames per window
                    x_bs = h_bs * upsampling_factor + 1                            # samples per window
                    h_ss = batch_length // upsampling_factor                       # window stride
                    x_ss = h_ss * upsampling_factor
                    more = lambda: len(h_buffer) > h_bs                            # noqa: E731
                else:
                    x_bs = h_bs = receptive_field + batch_length
                    x_ss = h_ss = batch_length
                    more = lambda: len(x_buffer) > x_bs                            # noqa: E731
                while more():
                    if my_lo <= n_in_batch < my_hi:   # windows of other ranks are only skipped over
                        if pre:
                            window_jobs.append(submit(prep, x_buffer[:x_bs], h_buffer[:h_bs], xt_buffer[:x_bs], ht_buffer[:h_bs]))
                        else:
                            window_jobs.append(submit(prep, x_buffer[:x_bs], h_buffer[:h_bs]))
                    n_in_batch += 1
                    h_buffer = h_buffer[h_ss:]
                    x_buffer = x_buffer[x_ss:]
                    if pre:
                        ht_buffer = ht_buffer[h_ss:]
                        xt_buffer = xt_buffer[x_ss:]
                    if n_in_batch == batch_size:
                        if window_jobs:
                            ready.append(submit(assemble, window_jobs))
                        window_jobs = []
                        n_in_batch = 0
                        while len(ready) >= max_ready:
                            yield ready.popleft().result()
            else:
                # one utterance per batch; with several ranks utterance i goes to rank i mod world
                n_seen += 1
                if not padded and shard is not None and (n_seen - 1) % shard[1] != shard[0]:
                    continue
                x, h, xt, ht = _whole_utterance(x, h, xt, ht, upsampling_factor, use_upsampling_layer)
                if padded:
                    # batch_size consecutive utterances per minibatch; rows of other ranks only contribute their length
                    if my_lo <= n_in_batch < my_hi:
                        window_jobs.append(submit(prep, x, h, xt, ht) if pre else submit(prep, x, h))
                    group_lengths.append(len(x) - 1)
                    n_in_batch += 1
                    if n_in_batch == batch_size:
                        ready.append(submit(assemble_padded, window_jobs, group_lengths, my_lo))
                        window_jobs = []
                        group_lengths = []
                        n_in_batch = 0
                        while len(ready) >= max_ready:
                            yield ready.popleft().result()
                    continue
                ready.append(submit(assemble, [submit(prep, x, h, xt, ht) if pre else submit(prep, x, h)]))
                while len(ready) >= max_ready:
                    yield ready.popleft().result()
    finally:
        if pool is not None:
            pool.shutdown(wait=False)


def evaluate_corpus(model, wav_list, feat_list, batch_size,
                    feature_type="world",
                    wav_transform=None,
                    feat_transform=None,
                    upsampling_factor=80,
                    use_upsampling_layer=True,
                    use_speaker_code=False,
                    device=None,
                    shard=None,
                    transforms_elementwise=False,
                    n_quantize=None,
                    length_cache=None):
    """Score every utterance of a list exactly once with ``model.evaluate`` (NOT a reference function: the reference has no
    held-out loss).  Feature, transform and upsampling arguments as ``train_generator``, whose reading and transform code this
    shares.

    The utterances are sorted by length (ties by list index: little padding, a deterministic order) and grouped ``batch_size`` at
    a time -- the last group may be smaller, nothing is dropped -- each group padded as ``train_generator(pad_utterances=True)``
    pads (tokens and targets ``n_quantize // 2``, the last frame repeated, a whole number of frames with the upsampling layer) and
    scored over the positions behind the receptive field.  ``shard=(rank, world)``: this rank takes the groups ``rank, rank +
    world, ...`` of the same grouping.  ``length_cache`` (a dict, optional): the lengths found by the first pass over the files
    are kept in it, so a later call with the same dict reads only the groups it scores.

    Returns ``(nll, positions, per_utterance, n_short)``: the total negative log-likelihood (accumulated on the device in double
    and read once at the end, with the per-utterance sums: the pass's only device-to-host synchronisation), the number of
    positions it covers, ``[(index, nll_sum, n_positions)]`` in list order for the utterances this call scored, and how many of
    them are not longer than the receptive field -- those have no position to score, count 0 and get one warning each.  The
    mean per position is ``nll / positions``; sums from several ranks or lists simply add."""
    eng = model.engine
    device = eng.device if device is None else torch.device(device)
    n_quantize = model.n_quantize if n_quantize is None else n_quantize
    rf = model.receptive_field
    pre = bool(transforms_elementwise)
    mixture = model.n_mixture > 0

    def load(i, transforms=True):
        utt = _load_utterance(wav_list[i], feat_list[i], feature_type, upsampling_factor, use_upsampling_layer, use_speaker_code,
                              wav_transform, feat_transform, pre and transforms)
        return _whole_utterance(*utt, upsampling_factor, use_upsampling_layer)

    n_lengths = []
    for i in range(len(wav_list)):
        key = (wav_list[i], feat_list[i])
        if length_cache is not None and key in length_cache:
            n_lengths.append(length_cache[key])
            continue
        n = max(len(load(i, transforms=False)[0]) - 1, 0)   # (the trimmed length alone: no mu-law, no scaler)
        if length_cache is not None:
            length_cache[key] = n
        n_lengths.append(n)
    order = sorted(range(len(wav_list)), key=lambda i: (n_lengths[i], i))
    groups = [order[g:g + batch_size] for g in range(0, len(order), batch_size)]
    if shard is not None:
        groups = groups[shard[0]::shard[1]]
    acc = torch.zeros(1, dtype=torch.float64, device=device)
    rows, scored, zeros, n_short = [], [], [], 0
    for group in groups:
        for i in group:
            if n_lengths[i] <= rf:
                n_short += 1
                logging.warning("%s is not longer than the receptive field (%d <= %d): no position to score."
                                % (wav_list[i], n_lengths[i], rf))
        empty = [i for i in group if n_lengths[i] < 1]   # (not a single input / target pair: nothing to run)
        group = [i for i in group if n_lengths[i] >= 1]
        zeros += [(i, 0.0, 0) for i in empty]
        if not group:
            continue
        windows = []
        for i in group:
            x, h, xt, ht = load(i)
            windows.append(_prep_window(x, h, xt, ht, wav_transform, feat_transform))
        xs, hs, ts, ys, lengths = _pad_rows(*_window_rows(windows, use_upsampling_layer), n_quantize)
        assert lengths.tolist() == [n_lengths[i] for i in group]
        if mixture:
            (bx, bh), _, by = _to_batch(xs, hs, ts, device, ys)
            row, counts = model.evaluate(bx, bh, y=by, lengths=lengths, acc=acc)
        else:
            (bx, bh), bt = _to_batch(xs, hs, ts, device)
            row, counts = model.evaluate(bx, bh, t=bt, lengths=lengths, acc=acc)
        rows.append(row)
        scored += list(zip(group, counts))
    values = torch.cat([acc] + [r.double() for r in rows]).cpu().tolist()   # the one read of the pass
    eng.release_eval_workspace()
    per_utt = sorted([(i, v, n) for (i, n), v in zip(scored, values[1:])] + zeros)
    return values[0], sum(n for _, n in scored), per_utt, n_short


def dev_loss(model, dev, rank, world, device):
    """One pass over the held-out list ``dev`` = (wav_list, feat_list, batch_size, keyword arguments of evaluate_corpus): every
    rank scores its shard, ONE all-reduce of the float64 pair [nll, positions]; returns (mean per position, utterances,
    positions) -- the same numbers on every rank."""
    import torch.distributed as dist
    wav_list, feat_list, batch_size, kw = dev
    nll, npos, per_utt, _ = evaluate_corpus(model, wav_list, feat_list, batch_size, device=device,
                                            shard=(rank, world) if world > 1 else None, **kw)
    pair = torch.tensor([nll, float(npos)], dtype=torch.float64, device=device)
    if world > 1:
        dist.all_reduce(pair)
    nll, npos = pair.tolist()
    return (nll / npos if npos > 0 else float("nan")), len(wav_list), int(npos)


def save_checkpoint(checkpoint_dir, model, optimizer, iterations, dev=None, adapters=None):
    """``checkpoint-%d.pkl`` = {"model", "optimizer", "iterations"} (reference train.py:315-332); with a held-out set
    (--dev_waveforms) also "dev" = {"best_loss", "best_iterations"}; with a moving average of the weights (--ema_decay) also
    "ema" = the averaged weights under the keys of "model".  With low-rank adapters (--adapter_rank) "adapter" takes the place of
    "model": the base stays in the --pretrained file."""
    checkpoint = {"model": model.state_dict(), "optimizer": optimizer.state_dict(), "iterations": iterations}
    if adapters is not None:
        checkpoint = {"adapter": adapters.state_dict(), "optimizer": optimizer.state_dict(), "iterations": iterations}
    if dev is not None:
        checkpoint["dev"] = dict(dev)
    if getattr(optimizer, "ema_decay", None) is not None:
        checkpoint["ema"] = optimizer.ema_state_dict()
    if not os.path.exists(checkpoint_dir):
        os.makedirs(checkpoint_dir)
    torch.save(checkpoint, checkpoint_dir + "/checkpoint-%d.pkl" % iterations)
    logging.info("%d-iter checkpoint created." % iterations)


def dev_best_state(dev_best):
    """The "dev" entry of a regular checkpoint from (lowest dev loss so far, its iteration); both None while no pass over the
    held-out set has given a finite loss yet (a checkpoint written in front of the first pass)."""
    return {"best_loss": dev_best[0] if dev_best else None, "best_iterations": dev_best[1] if dev_best else None}


def dev_best_from_checkpoint(checkpoint):
    """(lowest dev loss, its iteration) as --resume restores it, or None: a checkpoint of a run without a held-out set has no
    "dev" entry, one written in front of the first pass holds Nones."""
    state = checkpoint.get("dev") or {}
    if state.get("best_loss") is None or state.get("best_iterations") is None:
        return None
    return float(state["best_loss"]), int(state["best_iterations"])


# (flag, default, type, help) -- the reference's command line, train.py:339-393
_FLAGS = [
    # paths
    ("waveforms", argparse.SUPPRESS, str, "wav directory or .scp list"),
    ("feats", argparse.SUPPRESS, str, "aux-feature directory or .scp list"),
    ("stats", argparse.SUPPRESS, str, "statistics file (mean / scale per feature type)"),
    ("expdir", argparse.SUPPRESS, str, "output directory for model.conf and checkpoints"),
    # network
    ("n_quantize", 256, int, "mu-law levels"),
    ("n_aux", 28, int, "aux feature dimension"),
    ("n_resch", 512, int, "residual channels"),
    ("n_skipch", 256, int, "skip channels"),
    ("dilation_depth", 10, int, "dilations 1..2^(depth-1) per cycle"),
    ("dilation_repeat", 1, int, "number of dilation cycles"),
    ("kernel_size", 2, int, "taps of the dilated causal convolutions"),
    ("upsampling_factor", 80, int, "samples per aux frame"),
    ("use_upsampling_layer", True, strtobool, "learned upsampling layer (else features are repeated on the host)"),
    ("use_speaker_code", False, strtobool, "append /speaker_code to the features"),
    # optimisation
    ("lr", 1e-4, float, "Adam learning rate"),
    ("weight_decay", 0.0, float, "L2 coefficient"),
    ("batch_length", 20000, int, "loss-bearing samples per window"),
    ("batch_size", 1, int, "windows per minibatch (global, split across GPUs)"),
    ("iters", 200000, int, "training iterations"),
    # misc
    ("checkpoint_interval", 10000, int, "iterations between checkpoints"),
    ("intervals", 100, int, "iterations between log lines"),
    ("seed", 1, int, "random seed"),
    ("n_gpus", 1, int, "GPUs (one process each)"),
    ("verbose", 1, int, "0 warnings, 1 info, >1 debug"),
]


def get_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    for name, default, typ, text in _FLAGS:
        if default is argparse.SUPPRESS:
            parser.add_argument("--" + name, required=True, type=typ, help=text)
        else:
            parser.add_argument("--" + name, default=default, type=typ, help=text)
    parser.add_argument("--feature_type", default="world", choices=["world", "melspc"], type=str)
    # extension (not a reference flag): mixture-of-logistics output head with N components, 0 = softmax head
    parser.add_argument("--n_mixture", default=0, type=int, help="mixture-of-logistics components (0: softmax head)")
    parser.add_argument("--log_scale_min", default=-7.0, type=float,
                        help="mixture head: clamp of the log-scales (saved in model.conf, so decode.py samples with it)")
    # extension (not a reference flag): whole utterances, --batch_size of them per minibatch, padded to the longest one
    parser.add_argument("--utterance_batch", default=False, type=strtobool,
                        help="train on padded minibatches of --batch_size whole utterances (--batch_length is ignored)")
    # extensions (not reference flags): global-norm gradient clipping and the non-finite-step guard of FusedAdam, both on the
    # device (no synchronisation is added to the loop)
    parser.add_argument("--max_grad_norm", default=0.0, type=float,
                        help="clip the global gradient norm to this value before the Adam step (0: off)")
    parser.add_argument("--skip_nonfinite_steps", default=False, type=strtobool,
                        help="skip (and count) a step whose gradient holds a NaN or an inf instead of applying it")
    # extensions (not reference flags): a held-out set scored during training (evaluate_corpus); off without --dev_waveforms
    parser.add_argument("--dev_waveforms", default=None, type=str, help="held-out wav directory or .scp list (with --dev_feats)")
    parser.add_argument("--dev_feats", default=None, type=str, help="held-out aux-feature directory or .scp list")
    parser.add_argument("--eval_interval", default=0, type=int,
                        help="iterations between two passes over the held-out set (0: at every --checkpoint_interval)")
    parser.add_argument("--eval_batch_size", default=8, type=int, help="held-out utterances scored per padded batch")
    # extensions (not reference flags): an exponential moving average of the weights, updated inside the Adam launch
    parser.add_argument("--ema_decay", default=0.0, type=float,
                        help="decay of the moving average of the weights that the held-out set is scored with and "
                             "checkpoint-best.pkl holds (0: off)")
    parser.add_argument("--ema_warmup", default=True, type=strtobool,
                        help="decay min(ema_decay, (1 + t) / (10 + t)) at applied step t, so the average forgets the initial weights")
    # extension (not a reference flag): gradient accumulation -- A minibatches per optimizer step, their gradients summed on the
    # device (WaveNet.loss_and_backward(micro_step=)) and exchanged between ranks once
    parser.add_argument("--accum_steps", default=1, type=int,
                        help="minibatches per optimizer step (1: off); an iteration is one optimizer step and draws this many "
                             "minibatches.  The step is the mean over all their loss positions; one-utterance batches (whose "
                             "lengths the other ranks do not know) are weighted equally, 1 / (ranks * accum_steps)")
    parser.add_argument("--resume", default=None, nargs="?", type=str, help="checkpoint to continue from")
    # extension (not reference flags): fine-tuning part of a model (WaveNet.freeze / train_only)
    parser.add_argument("--pretrained", default=None, type=str,
                        help="checkpoint whose model weights start iteration 0 (fresh optimizer); not together with --resume")
    parser.add_argument("--freeze", default=None, type=str,
                        help="regular expression (re.search on the parameter names): the matching tensors are frozen")
    parser.add_argument("--train_only", default=None, type=str,
                        help="regular expression: only the matching tensors train, every other one is frozen; not together with --freeze")
    # extension (not a reference flag): parameter groups of FusedAdam
    parser.add_argument("--param_group", default=None, action="append", type=str, metavar="REGEX:KEY=VALUE[,KEY=VALUE...]",
                        help="repeatable: the tensors whose name matches REGEX (re.search; the first matching group wins) get "
                             "their own lr=, weight_decay=, eps= and decoupled=true|false (AdamW's decay); a missing key takes "
                             "--lr / --weight_decay.  Give the same groups with --resume: the checkpoint's values then win")
    # extension (not reference flags): layer-wise adaptive steps of FusedAdam (LAMB) for large batches
    parser.add_argument("--layer_adaptation", default=False, type=strtobool,
                        help="scale every adapted tensor's step by its trust ratio ||w|| / ||update||; tensors with two or more "
                             "dimensions adapt, biases do not (--param_group 'REGEX:adapt=true|false' overrides that per group)")
    parser.add_argument("--max_trust_ratio", default=0.0, type=float, help="upper bound of the trust ratio (0: none)")
    # extension (not reference flags): knowledge distillation from a trained model
    parser.add_argument("--teacher", default=None, type=str,
                        help="checkpoint of a trained softmax-head model whose output distribution the model is trained against "
                             "(its \"model\" weights; with --teacher_config)")
    parser.add_argument("--teacher_config", default=None, type=str, help="the model.conf the teacher's run saved")
    parser.add_argument("--distill_alpha", default=0.5, type=float,
                        help="weight of the teacher term in [0, 1]: loss = (1 - alpha) * ce + alpha * T^2 * kl")
    parser.add_argument("--distill_temperature", default=1.0, type=float, help="softmax temperature T > 0 of the teacher term")
    # extension (not reference flags): torch's CrossEntropyLoss(weight=, label_smoothing=) in the HIP step
    parser.add_argument("--label_smoothing", default=0.0, type=float,
                        help="label smoothing E in [0, 1) of the softmax head's criterion (0: none)")
    parser.add_argument("--class_weights", default=None, type=str,
                        help="a .npy or text file of n_quantize floats, finite and >= 0: one weight per class of the criterion")
    parser.add_argument("--loss_normalize", default="weights", type=str,
                        help="weights: divide the weighted loss by the sum of the targets' weights (torch's mean); positions: by "
                             "the number of loss positions (exact over ranks, --accum_steps and uneven batches)")
    # extension (not reference flags): low-rank adapters on a pretrained model: one base, a small file per voice
    parser.add_argument("--adapter_rank", default=0, type=int,
                        help="train low-rank adapters W0 + (alpha / rank) B A of this rank on the --pretrained model instead of its "
                             "weights (0: off); checkpoints then hold \"adapter\" and no \"model\"")
    parser.add_argument("--adapter_alpha", default=None, type=float, help="adapter scale numerator (default: the rank, scale 1)")
    parser.add_argument("--adapter_targets", default=None, type=str,
                        help="regular expression (re.search on the parameter names) of the adapted weights; default: the dilated, "
                             "skip and residual convolutions of every layer")
    parser.add_argument("--adapter_save_merged", default=False, type=strtobool,
                        help="checkpoint-final.pkl also holds \"model\", the merged weights, for tools that know no adapters")
    return parser


def check_adapter_args(args):
    """The refusals of --adapter_rank, made while main() looks at the arguments.  ValueError with the reason."""
    rank = int(getattr(args, "adapter_rank", 0) or 0)
    if rank < 0:
        raise ValueError("--adapter_rank %d: a positive rank, or 0 for none." % rank)
    if rank == 0:
        for flag in ("adapter_alpha", "adapter_targets", "adapter_save_merged"):
            if getattr(args, flag, None):
                raise ValueError("--%s needs --adapter_rank." % flag)
        if args.pretrained and args.resume:
            raise ValueError("--pretrained starts iteration 0 from a checkpoint's weights, --resume continues a run: give one of "
                             "them (both only with --adapter_rank: the base from one file, the adapters from the other).")
        return
    if not args.pretrained:
        raise ValueError("--adapter_rank needs --pretrained: adapters are trained on a trained model.")
    for flag, on in (("--freeze", bool(args.freeze)), ("--train_only", bool(args.train_only)),
                     ("--ema_decay", float(args.ema_decay or 0.0) > 0.0), ("--param_group", bool(args.param_group)),
                     ("--layer_adaptation", bool(args.layer_adaptation))):
        if on:
            raise ValueError("--adapter_rank cannot go with %s: the adapters are the trainable set, and the weight average, "
                             "parameter groups and layer adaptation are not defined for them." % flag)


def check_criterion_args(args):
    """The refusals of --label_smoothing / --class_weights / --loss_normalize, made while main() looks at the arguments; returns
    the class weights as a host float32 tensor (None: no --class_weights).  ValueError with the reason."""
    eps, path = float(getattr(args, "label_smoothing", 0.0)), getattr(args, "class_weights", None)
    normalize = getattr(args, "loss_normalize", "weights")
    if normalize not in ("weights", "positions"):
        raise ValueError("--loss_normalize %s: weights or positions." % normalize)
    if not 0.0 <= eps < 1.0:
        raise ValueError("--label_smoothing %g is outside [0, 1)." % eps)
    if not path and eps == 0.0:
        return None
    for flag, on in (("--label_smoothing", eps != 0.0), ("--class_weights", bool(path))):
        if on and args.n_mixture > 0:
            raise ValueError("%s needs the softmax head: the criterion's options are not defined for --n_mixture %d." % (flag, args.n_mixture))
        if on and getattr(args, "teacher", None):
            raise ValueError("%s cannot go with --teacher: the distillation loss has no such option." % flag)
    if not path:
        return None
    if not os.path.isfile(path):
        raise ValueError("--class_weights %s does not exist." % path)
    try:
        values = np.load(path) if path.endswith(".npy") else np.loadtxt(path)
        weights = torch.as_tensor(np.asarray(values, dtype=np.float64).reshape(-1))
    except (ValueError, OSError) as err:
        raise ValueError("--class_weights %s cannot be read as floats: %s" % (path, err))
    if weights.numel() != args.n_quantize:
        raise ValueError("--class_weights %s holds %d values, the model has n_quantize = %d classes." % (path, weights.numel(), args.n_quantize))
    if not bool(torch.isfinite(weights).all()) or bool((weights < 0).any()):
        raise ValueError("--class_weights %s: every weight must be finite and >= 0." % path)
    return weights.float()


TEACHER_MUST_MATCH = ("n_quantize", "n_aux", "upsampling_factor", "use_upsampling_layer")


def check_teacher_args(args):
    """The refusals of --teacher, made while main() looks at the arguments; returns the teacher's configuration (None: no
    teacher).  ValueError with the reason."""
    teacher, conf = getattr(args, "teacher", None), getattr(args, "teacher_config", None)
    if not teacher and not conf:
        return None
    if not teacher or not conf:
        raise ValueError("--teacher and --teacher_config go together: the checkpoint holds no model configuration.")
    if args.n_mixture > 0:
        raise ValueError("--teacher needs the softmax head: distillation is not defined for --n_mixture %d." % args.n_mixture)
    alpha, temperature = float(args.distill_alpha), float(args.distill_temperature)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("--distill_alpha %g is outside [0, 1]." % alpha)
    if not (temperature > 0.0 and temperature < float("inf")):
        raise ValueError("--distill_temperature %g must be positive and finite." % temperature)
    for path, flag in ((conf, "--teacher_config"), (teacher, "--teacher")):
        if not os.path.isfile(path):
            raise ValueError("%s %s does not exist." % (flag, path))
    config = torch.load(conf, weights_only=False)
    if getattr(config, "n_mixture", 0) > 0:
        raise ValueError("--teacher_config %s describes a mixture-of-logistics model: the teacher needs the softmax head." % conf)
    for key in TEACHER_MUST_MATCH:
        if getattr(config, key) != getattr(args, key):
            raise ValueError("the teacher's %s (%s) differs from the model's (%s): the two must read the same inputs and share the "
                             "classes." % (key, getattr(config, key), getattr(args, key)))
    return config


def build_teacher(config, checkpoint, device):
    """The teacher of --teacher: built from its run's model.conf, its "model" weights loaded (a checkpoint-best.pkl contributes
    its averaged weights), on the rank's device, never trained.  The global random state is left as it was."""
    with torch.random.fork_rng(devices=[]):
        teacher = WaveNet(n_quantize=config.n_quantize, n_aux=config.n_aux, n_resch=config.n_resch, n_skipch=config.n_skipch,
                          dilation_depth=config.dilation_depth, dilation_repeat=config.dilation_repeat,
                          kernel_size=config.kernel_size,
                          upsampling_factor=config.upsampling_factor if config.use_upsampling_layer else 0)
    teacher.load_state_dict(torch.load(checkpoint, map_location=lambda storage, loc: storage, weights_only=False)["model"])
    teacher.requires_grad_(False)
    teacher.eval()
    teacher.to(device)
    return teacher


PARAM_GROUP_KEYS = {"lr": "lr", "weight_decay": "weight_decay", "eps": "eps", "decoupled": "decoupled_weight_decay",
                    "adapt": "layer_adaptation"}


def parse_param_group(spec):
    """``'REGEX:lr=3e-4,weight_decay=0,eps=1e-6,decoupled=true'`` -> ``(regex, dict)`` as ``FusedAdam(groups=)`` takes it.  The
    values stand behind the LAST colon (a regex may hold one); ValueError with the reason for anything else."""
    pattern, colon, values = spec.rpartition(":")
    if not colon or not pattern or not values:
        raise ValueError("--param_group %r: expected REGEX:KEY=VALUE[,KEY=VALUE...]" % spec)
    try:
        re.compile(pattern)
    except re.error as err:
        raise ValueError("--param_group %r: bad regular expression (%s)" % (spec, err))
    out = {}
    for item in values.split(","):
        key, eq, value = item.partition("=")
        key = key.strip()
        if not eq or key not in PARAM_GROUP_KEYS:
            raise ValueError("--param_group %r: %r is not one of %s=VALUE" % (spec, item, ", ".join(sorted(PARAM_GROUP_KEYS))))
        try:
            out[PARAM_GROUP_KEYS[key]] = bool(strtobool(value.strip())) if key in ("decoupled", "adapt") else float(value)
        except ValueError:
            raise ValueError("--param_group %r: bad value in %r" % (spec, item))
    return pattern, out


def _file_lists(waveforms, feats, flag):
    """wav / feature file lists from a directory or a list file (reference train.py:472-482)"""
    if os.path.isdir(waveforms):
        filenames = sorted(find_files(waveforms, "*.wav", use_dir_name=False))
        return ([waveforms + "/" + filename for filename in filenames],
                [feats + "/" + filename.replace(".wav", ".h5") for filename in filenames])
    if os.path.isfile(waveforms):
        return read_txt(waveforms), read_txt(feats)
    logging.error("%s should be directory or list." % flag)
    sys.exit(1)


def _fmt_eta(seconds):
    seconds = int(seconds)
    days, rem = divmod(seconds, 86400)
    hours, rem = divmod(rem, 3600)
    minutes, secs = divmod(rem, 60)
    return "%02d:%02d:%02d:%02d" % (days, hours, minutes, secs)


def _worker(rank, world, args, port):
    """One training process (one GPU)."""
    import torch.distributed as dist
    from pytorchwavenetvocoder_amd.distributed import GradientReducer
    from pytorchwavenetvocoder_amd.optim import FusedAdam

    level = logging.INFO if args.verbose == 1 else logging.DEBUG if args.verbose > 1 else logging.WARNING
    logging.basicConfig(level=level, format='%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s',
                        datefmt='%m/%d/%Y %I:%M:%S')
    if args.verbose < 1:
        logging.warning("logging is disabled.")
    if not torch.cuda.is_available():
        logging.error("gpu is not available. please check the setting.")  # reference train.py:524-525
        sys.exit(1)
    # WN_TRAIN_BACKEND=gloo lets the N-rank control flow (sharded slicer, bucketed exchange, identical Adam) be exercised on a box
    # with fewer GPUs than ranks -- the ranks then share devices; real runs use nccl (= RCCL), one rank per GPU.
    backend = os.environ.get("WN_TRAIN_BACKEND", "nccl")
    dev_index = rank if backend == "nccl" else rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(port))
        if backend == "nccl":
            from pytorchwavenetvocoder_amd.distributed import rccl_footprint_defaults
            rccl_footprint_defaults()
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    is_main = rank == 0
    if is_main:
        for key, value in vars(args).items():
            logging.info("%s = %s" % (key, str(value)))
        if not os.path.exists(args.expdir):
            os.makedirs(args.expdir)

    # fix seed (identical on every rank: same shuffles, same initial weights)
    os.environ['PYTHONHASHSEED'] = str(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if is_main:
        torch.save(args, args.expdir + "/model.conf")

    upsampling_factor = args.upsampling_factor if args.use_upsampling_layer else 0
    model = WaveNet(n_quantize=args.n_quantize, n_aux=args.n_aux, n_resch=args.n_resch, n_skipch=args.n_skipch,
                    dilation_depth=args.dilation_depth, dilation_repeat=args.dilation_repeat,
                    kernel_size=args.kernel_size, upsampling_factor=upsampling_factor, n_mixture=args.n_mixture,
                    log_scale_min=args.log_scale_min)
    if is_main:
        logging.info(model)
    model.apply(initialize)
    model.train()
    if world > args.batch_size:
        logging.warning("batch size is less than number of gpus.")

    # transforms (reference: StandardScaler + mu-law, train.py:464-470)
    mean = read_hdf5(args.stats, "/" + args.feature_type + "/mean")
    scale = read_hdf5(args.stats, "/" + args.feature_type + "/scale")
    wav_transform = lambda x: encode_mu_law(x, args.n_quantize)   # noqa: E731
    feat_transform = make_feat_transform(mean, scale)

    wav_list, feat_list = _file_lists(args.waveforms, args.feats, "--waveforms")
    assert len(wav_list) == len(feat_list)
    logging.info("number of training data = %d." % len(wav_list))
    utterance_batch = bool(getattr(args, "utterance_batch", False))
    # --teacher: windows carry the context of the deeper of the two models, and the loss starts behind it
    teacher, rf = None, model.receptive_field
    if getattr(args, "teacher", None):
        teacher = build_teacher(check_teacher_args(args), args.teacher, device)   # (main() has made the refusals)
        rf = max(model.receptive_field, teacher.receptive_field)
        distill_alpha, distill_temperature = float(args.distill_alpha), float(args.distill_temperature)
        logging.info("teacher from %s: receptive field %d (the model's: %d), alpha %g, temperature %g." % (
            args.teacher, teacher.receptive_field, model.receptive_field, distill_alpha, distill_temperature))
    generator = train_generator(
        wav_list, feat_list,
        receptive_field=rf,
        batch_length=None if utterance_batch else args.batch_length,
        batch_size=args.batch_size,
        pad_utterances=utterance_batch,
        n_quantize=args.n_quantize,
        feature_type=args.feature_type,
        wav_transform=wav_transform,
        feat_transform=feat_transform,
        shuffle=True,
        upsampling_factor=args.upsampling_factor,
        use_upsampling_layer=args.use_upsampling_layer,
        shard=(rank, world) if world > 1 else None,
        with_wave=args.n_mixture > 0,
        use_speaker_code=args.use_speaker_code,
        device=device,
        transforms_elementwise=True)   # mu-law and the standard scaler are per-sample / per-frame maps

    dev, dev_best = None, None   # held-out set (off without --dev_waveforms); (lowest dev loss so far, its iteration)
    if getattr(args, "dev_waveforms", None):
        if not getattr(args, "dev_feats", None):
            logging.error("--dev_waveforms needs --dev_feats.")
            sys.exit(1)
        dev_wav, dev_feat = _file_lists(args.dev_waveforms, args.dev_feats, "--dev_waveforms")
        assert len(dev_wav) == len(dev_feat)
        logging.info("number of held-out data = %d." % len(dev_wav))
        dev = (dev_wav, dev_feat, max(1, int(args.eval_batch_size)),
               dict(feature_type=args.feature_type, wav_transform=wav_transform, feat_transform=feat_transform,
                    upsampling_factor=args.upsampling_factor, use_upsampling_layer=args.use_upsampling_layer,
                    use_speaker_code=args.use_speaker_code, transforms_elementwise=True, n_quantize=args.n_quantize,
                    length_cache={}))
    eval_interval = (int(getattr(args, "eval_interval", 0)) or args.checkpoint_interval) if dev is not None else 0

    max_grad_norm = float(getattr(args, "max_grad_norm", 0.0) or 0.0)
    ema_decay = float(getattr(args, "ema_decay", 0.0) or 0.0)
    groups = [parse_param_group(spec) for spec in (getattr(args, "param_group", None) or [])]   # (main() has checked the syntax)
    layer_adaptation = bool(getattr(args, "layer_adaptation", False))
    max_trust_ratio = float(getattr(args, "max_trust_ratio", 0.0) or 0.0)
    lamb = {"layer_adaptation": True, "max_trust_ratio": max_trust_ratio if max_trust_ratio > 0.0 else None} if layer_adaptation else {}
    adapter_rank, adapters = int(getattr(args, "adapter_rank", 0) or 0), None
    try:
        optimizer = None if adapter_rank > 0 else \
                    FusedAdam(model, lr=args.lr, weight_decay=args.weight_decay,
                              max_grad_norm=max_grad_norm if max_grad_norm > 0.0 else None,
                              skip_nonfinite=bool(getattr(args, "skip_nonfinite_steps", False)),
                              ema_decay=ema_decay if ema_decay > 0.0 else None, ema_warmup=bool(getattr(args, "ema_warmup", True)),
                              **dict({"groups": groups} if groups else {}, **lamb))   # noqa: E127
    except ValueError as err:
        if not groups:
            raise
        logging.error("--param_group: %s" % err)
        sys.exit(1)
    if layer_adaptation:
        logging.info("layer-wise adaptive steps: tensors with two or more dimensions adapt, max trust ratio %s%s" % (
            "%g" % max_trust_ratio if max_trust_ratio > 0.0 else "none",
            "".join("; group %d (%r) adapt=%s" % (i, groups[i - 1][0], g["layer_adaptation"])
                    for i, g in enumerate(optimizer.param_groups) if "layer_adaptation" in g)))
    for i, g in enumerate(optimizer.param_groups if groups and optimizer is not None else []):
        logging.info("parameter group %d (%s): lr=%g weight_decay=%g eps=%g decoupled=%s, %d tensors, %d elements" % (
            i, "default" if i == 0 else repr(groups[i - 1][0]), g["lr"], g["weight_decay"], g["eps"],
            bool(g["decoupled_weight_decay"]), len(g["params"]), sum(p.numel() for p in g["params"])))
    pretrained, freeze, train_only = (getattr(args, k, None) or None for k in ("pretrained", "freeze", "train_only"))
    if pretrained:   # (main() has refused --pretrained beside --resume and --freeze beside --train_only)
        model.load_state_dict(torch.load(pretrained, map_location=lambda storage, loc: storage, weights_only=False)["model"])
        logging.info("model weights from %s (iteration 0, fresh optimizer)." % pretrained)
    if adapter_rank > 0:   # (main() has made the refusals) the adapters become the trainable set; the base stays as loaded
        try:
            adapters = LowRankAdapters(model, rank=adapter_rank, alpha=getattr(args, "adapter_alpha", None),
                                       targets=getattr(args, "adapter_targets", None) or None, seed=args.seed)
        except (ValueError, re.error) as err:
            logging.error("--adapter_rank / --adapter_targets: %s" % err)
            sys.exit(1)
        optimizer = AdapterAdam(adapters, lr=args.lr, weight_decay=args.weight_decay,
                                max_grad_norm=max_grad_norm if max_grad_norm > 0.0 else None,
                                skip_nonfinite=bool(getattr(args, "skip_nonfinite_steps", False)))
        logging.info("low-rank adapters: rank %d, alpha %g, %d tensors, %d adapter parameters (the model has %d)" % (
            adapters.rank, adapters.alpha, len(adapters.entries), adapters.n_adapter, sum(p.numel() for p in model.parameters())))
    if freeze or train_only:
        if freeze:
            model.freeze(freeze)
        else:
            model.train_only(train_only)
        tensors = list(model.parameters())
        frozen = [p for p in tensors if not p.requires_grad]
        logging.info("trainable parameters = %d of %d (%d of %d tensors frozen)" % (
            sum(p.numel() for p in tensors) - sum(p.numel() for p in frozen), sum(p.numel() for p in tensors), len(frozen), len(tensors)))
    if args.resume is not None and len(args.resume) != 0:
        checkpoint = torch.load(args.resume, map_location=lambda storage, loc: storage, weights_only=False)
        iterations = checkpoint["iterations"]
        if adapters is not None:   # the base came from --pretrained, the adapters and their optimizer come from this file
            try:
                if "adapter" not in checkpoint:
                    raise ValueError("%s holds no \"adapter\" entry (it was not written by a run with --adapter_rank)" % args.resume)
                adapters.load_state_dict(checkpoint["adapter"])
            except ValueError as err:
                logging.error("--resume: %s" % err)
                sys.exit(1)
        else:
            model.load_state_dict(checkpoint["model"])
        optimizer.load_state_dict(checkpoint["optimizer"])
        if dev is not None:
            dev_best = dev_best_from_checkpoint(checkpoint)
        if optimizer.ema_decay is not None:
            if "ema" in checkpoint:
                optimizer.load_ema_state_dict(checkpoint["ema"])
            else:
                logging.warning("the checkpoint holds no moving average (\"ema\"): it starts from the model weights.")
        logging.info("restored from %d-iter checkpoint." % iterations)
    else:
        iterations = 0
    model.to(device)
    reducer = GradientReducer(model)
    if world > 1:
        dist.broadcast(model.engine.flat_params, src=0)
    if adapters is not None:
        adapters.merge()   # the model holds the merged weights from here on (fresh adapters: the pretrained ones, B = 0)

    loss_acc = torch.zeros(1, device=device)
    # --label_smoothing / --class_weights: the weighted criterion (main() has made the refusals); its plain cross-entropy part is logged
    class_weights, label_smoothing = check_criterion_args(args), float(getattr(args, "label_smoothing", 0.0))
    weighted = class_weights is not None or label_smoothing != 0.0
    if weighted:
        class_weights = None if class_weights is None else class_weights.to(device)
        logging.info("criterion: label smoothing %g, class weights from %s, normalized by %s." % (
            label_smoothing, getattr(args, "class_weights", None), args.loss_normalize))
    ce_acc = torch.zeros(1, device=device) if weighted else None
    distilling = teacher is not None and distill_alpha != 0.0   # (alpha == 0: the teacher has no say, the step is the plain one)
    parts_acc = torch.zeros(3, device=device) if distilling else None   # the total, its cross-entropy and its (unweighted) kl part
    norm_acc = torch.zeros(1, device=device)     # guarded optimizer: sum of the finite pre-clip gradient norms of the interval
    skipped_seen = optimizer.steps_skipped()
    total = 0.0
    accum_steps = int(getattr(args, "accum_steps", 1) or 1)
    if accum_steps < 1:
        logging.error("--accum_steps must be at least 1.")
        sys.exit(1)

    def shares_of(items):
        """Per minibatch of one optimizer step: (this rank's share of the step's loss positions, the ``lengths=`` keyword)."""
        out = []
        for item in items:
            batch_x = item[0][0]
            # A rank's loss is the mean over ITS windows: weighting it (and its gradients) by B_local / batch_size makes the
            # sum over ranks the mean over the whole minibatch -- what the reference's single CrossEntropyLoss over the
            # gathered logits computes (train.py:534-536) -- also when batch_size is not a multiple of the rank count.
            share = batch_x.size(0) / float(args.batch_size) if (world > 1 and args.batch_length is not None) else 1.0 / world
            ragged, n_global = {}, None
            if utterance_batch and args.batch_size > 1:
                # padded whole utterances: the loss is the mean over the valid positions behind the receptive field.  This rank's
                # share of the minibatch is N_local / N_global loss positions (every rank knows every length: no communication).
                lengths, all_lengths = item[-2], item[-1]
                n_local = int((lengths - rf).clamp_(min=0).sum())
                n_global = int((all_lengths - rf).clamp_(min=0).sum())
                ragged["lengths"] = lengths
                share = n_local / float(max(n_global, 1))
            out.append([share, ragged, n_global])
        if len(items) > 1:
            # --accum_steps: the step's loss is the mean over the loss positions of ALL its micro-batches.  Padded utterance
            # batches: N_local,i / sum_j N_global,j.  Windows (equal counts) and single utterances (lengths unknown to the other
            # ranks: weighted equally, as the ranks are): the minibatch's own share / A.
            n_step = sum(o[2] for o in out) if out[0][2] is not None else None
            for o in out:
                o[0] = o[0] * o[2] / float(max(n_step, 1)) if n_step is not None else o[0] / len(items)
        return out

    for i in range(iterations, args.iters):
        start = time.time()
        items = [generator.next() for _ in range(accum_steps)]   # drawn first, then run as micro-steps (k, A)
        for k, (item, (share, ragged, _)) in enumerate(zip(items, shares_of(items))):
            (batch_x, batch_h), batch_t = item[0], item[1]
            if accum_steps > 1:
                ragged["micro_step"] = (k, accum_steps)
            if teacher is not None:
                ragged["t_start"] = rf
            if distilling:   # the teacher's forward on this rank's own micro-batch, then the student's step with its logits
                ragged.update(teacher_logits=teacher.teacher_logits(batch_x, batch_h), distill_alpha=distill_alpha,
                              distill_temperature=distill_temperature)
            if weighted:
                ragged.update(class_weights=class_weights, label_smoothing=label_smoothing, normalize=args.loss_normalize)
            batch_loss = reducer.loss_and_backward(batch_x, batch_h, batch_t, y=item[2] if args.n_mixture > 0 else None,
                                                   grad_scale=share, **ragged)
            if k == accum_steps - 1:
                if adapters is not None:   # behind the reduction: every rank projects the same reduced dW
                    adapters.project()
                optimizer.step()
            loss_acc += batch_loss.detach() * (share * world)
            if distilling:
                parts_acc += model.distill_parts.detach() * (share * world)
            if weighted:
                ce_acc += model.criterion_parts[1:2].detach() * (share * world)
        if optimizer.guarded:   # device-side accumulation, read at the interval's synchronisation below
            norm_acc += torch.nan_to_num(optimizer.grad_norm, nan=0.0, posinf=0.0)
        if args.verbose > 1:
            logging.debug("batch loss = %.3f (%.3f sec / batch)" % (batch_loss.item(), time.time() - start))
        total += time.time() - start

        if (i + 1) % args.intervals == 0:
            torch.cuda.synchronize(device)
            if world > 1:
                dist.all_reduce(loss_acc)
                loss_acc /= world
                if distilling:
                    dist.all_reduce(parts_acc)
                    parts_acc /= world
                if weighted:
                    dist.all_reduce(ce_acc)
                    ce_acc /= world
            if is_main:
                logging.info("(iter:%d) average loss = %.6f (%.3f sec / batch)" % (
                    i + 1, loss_acc.item() / args.intervals, total / args.intervals))
                if distilling:
                    parts = (parts_acc / args.intervals).tolist()
                    logging.info("(iter:%d) average ce = %.6f, average kl = %.6f (alpha %g, temperature %g)" % (
                        i + 1, parts[1], parts[2], distill_alpha, distill_temperature))
                if weighted:
                    logging.info("(iter:%d) average ce = %.6f (label smoothing %g, normalized by %s)" % (
                        i + 1, ce_acc.item() / args.intervals, label_smoothing, args.loss_normalize))
                logging.info("estimated required time = " + _fmt_eta((args.iters - (i + 1)) * (total / args.intervals)))
            if optimizer.guarded:
                # every rank holds the same reduced gradient, hence the same norm: nothing to exchange
                skipped_total = optimizer.steps_skipped()
                skipped, skipped_seen = skipped_total - skipped_seen, skipped_total
                if is_main:
                    finite = max(args.intervals - skipped, 1)   # a skipped step's norm is not finite: it is left out of the mean
                    logging.info("(iter:%d) average gradient norm before clipping = %.6f, skipped steps = %d" % (
                        i + 1, norm_acc.item() / finite, skipped))
                norm_acc.zero_()
            if layer_adaptation and is_main and any(optimizer.tensor_adapts or ()):
                # one read, here only: every rank derives the same ratios (the step needs none of them on the host)
                ratios = optimizer.trust_ratios.cpu()[torch.tensor(optimizer.tensor_adapts)]
                logging.info("(iter:%d) trust ratio min = %.4g, median = %.4g, max = %.4g (%d adapted tensors)" % (
                    i + 1, ratios.min().item(), ratios.median().item(), ratios.max().item(), ratios.numel()))
            loss_acc.zero_()
            if distilling:
                parts_acc.zero_()
            if weighted:
                ce_acc.zero_()
            total = 0.0
        if eval_interval > 0 and (i + 1) % eval_interval == 0:
            # every rank scores its shard of the held-out list; one all-reduce of [nll, positions] makes the mean
            start = time.time()
            # with a moving average the pass scores the AVERAGED weights, and those are what checkpoint-best.pkl keeps
            with (optimizer.ema_weights() if optimizer.ema_decay is not None else contextlib.nullcontext()):
                loss_dev, n_utt, n_pos = dev_loss(model, dev, rank, world, device)
            if is_main:
                if optimizer.ema_decay is not None:
                    logging.info("(iter:%d) the dev loss is that of the averaged weights (ema_decay %g)." % (i + 1, ema_decay))
                logging.info("(iter:%d) dev loss = %.6f (%d utterances, %d samples, %.3f sec)" % (
                    i + 1, loss_dev, n_utt, n_pos, time.time() - start))
                with open(args.expdir + "/dev_loss.txt", "a") as fh:
                    fh.write("%d %.6f %d %d\n" % (i + 1, loss_dev, n_utt, n_pos))
            if loss_dev == loss_dev and (dev_best is None or loss_dev < dev_best[0]):   # (same numbers on every rank)
                dev_best = (loss_dev, i + 1)
                if is_main:
                    best = {"model": model.state_dict(), "iterations": i + 1, "dev_loss": loss_dev}
                    if adapters is not None:   # what was scored is base + adapters: the small file, the merged weights on request
                        best = {"adapter": adapters.state_dict(), "iterations": i + 1, "dev_loss": loss_dev}
                        if getattr(args, "adapter_save_merged", False):
                            best["model"] = model.state_dict()
                    if optimizer.ema_decay is not None:   # "model" = what was scored: the reference's decode tool reads it as it is
                        best["model"] = optimizer.ema_state_dict()
                        best["ema_decay"] = ema_decay
                    torch.save(best, args.expdir + "/checkpoint-best.pkl")
                    logging.info("best checkpoint created (dev loss %.6f)." % loss_dev)
        if (i + 1) % args.checkpoint_interval == 0 and is_main:
            if dev is None:
                save_checkpoint(args.expdir, model, optimizer, i + 1, adapters=adapters)
            else:
                save_checkpoint(args.expdir, model, optimizer, i + 1, dev=dev_best_state(dev_best), adapters=adapters)

    generator.close()   # stop the producer thread before the interpreter tears the runtime down under it
    if is_main:
        final = {"model": model.state_dict()}
        if adapters is not None:
            final = {"adapter": adapters.state_dict()}
            if getattr(args, "adapter_save_merged", False):
                final["model"] = model.state_dict()
        if optimizer.ema_decay is not None:
            final["ema"] = optimizer.ema_state_dict()
        torch.save(final, args.expdir + "/checkpoint-final.pkl")
        logging.info("final checkpoint created.")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main(argv=None):
    """RUN TRAINING."""
    args = get_parser().parse_args(argv)
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    n_ranks = world_env if world_env > 1 else args.n_gpus
    if n_ranks > 1 and (args.batch_length is not None or args.utterance_batch) and args.batch_size < n_ranks:
        # every rank must own at least one window of each minibatch (the reference scatters the same way)
        logging.error("--batch_size (%d) must be >= the number of GPUs (%d)." % (args.batch_size, n_ranks))
        sys.exit(1)
    if args.freeze and args.train_only:
        logging.error("--freeze and --train_only exclude each other.")
        sys.exit(1)
    try:
        for spec in args.param_group or []:
            parse_param_group(spec)
    except ValueError as err:
        logging.error(str(err))
        sys.exit(1)
    if args.max_trust_ratio < 0.0 or (args.max_trust_ratio > 0.0 and not args.layer_adaptation):
        logging.error("--max_trust_ratio takes a positive bound and needs --layer_adaptation true.")
        sys.exit(1)
    if not args.layer_adaptation and any("layer_adaptation" in parse_param_group(spec)[1] for spec in args.param_group or []):
        logging.error("--param_group ...:adapt= needs --layer_adaptation true.")
        sys.exit(1)
    try:
        check_adapter_args(args)
        check_teacher_args(args)
        check_criterion_args(args)
    except ValueError as err:
        logging.error(str(err))
        sys.exit(1)
    if world_env > 1:  # launched by torch.distributed.run: one process per GPU already
        _worker(int(os.environ.get("LOCAL_RANK", os.environ.get("RANK", "0"))), world_env, args,
                int(os.environ.get("MASTER_PORT", "29500")))
    elif args.n_gpus > 1:
        import socket
        import torch.multiprocessing as mp
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        mp.spawn(_worker, args=(args.n_gpus, args, port), nprocs=args.n_gpus, join=True)
    else:
        _worker(0, 1, args, 0)


if __name__ == "__main__":
    main()
