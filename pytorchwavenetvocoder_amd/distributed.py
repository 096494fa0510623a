# -*- coding: utf-8 -*-
"""Data-parallel gradient reduction: one process per GPU, RCCL all-reduce over xGMI.

Replaces the reference's single-process ``torch.nn.DataParallel`` (train.py:449-454: per-step
parameter broadcast, logits gather to GPU0, gradient reduce to GPU0) with the minimum exchange the
path needs: every rank computes its own loss on its own shard of the minibatch and ONE flat fp32
gradient buffer is summed across ranks (gradients are pre-scaled by 1/world_size inside the loss
kernel, so the sum is the global-batch mean the reference's loss produces).  The buffer is laid
out in backward-completion order, so buckets are contiguous ranges: ``wn_backward`` records a HIP
event after each bucket and the all-reduce of bucket i runs on a side stream while the backward
kernels of the following layers are still executing.
"""
import os

import torch
import torch.distributed as dist

from ._lib import ACCUM_FINISH as _ACCUM_FINISH


def rccl_footprint_defaults():
    """Call before ``init_process_group("nccl")``.  The fused chain kernels are persistent grids that need a whole CU
    per workgroup (120 KB LDS, every VGPR); for the benchmark geometry they use 240 of the 256 CUs.  An RCCL kernel
    with more workgroups (= channels) than the 16 CUs left would take CUs a chain kernel is about to claim, and the
    unplaced part of that grid only starts when the rest of it retires (measured with a side-stream contraction:
    DESIGN.md 5.1).  The gradient buffer is 6.4 MB in 4 buckets -- latency-bound, so 16 channels cost nothing.
    ``setdefault``: an explicit NCCL_MAX_NCHANNELS in the environment wins."""
    os.environ.setdefault("NCCL_MAX_NCHANNELS", "16")


class GradientReducer(object):
    """Bucketed all-reduce of the flat gradient buffer beside the backward kernels.

    ``loss_and_backward`` returns after the caller's stream has joined the side stream, so what ``FusedAdam.step()`` reads is
    already the GLOBAL gradient.  With ``FusedAdam(max_grad_norm=...)`` / ``skip_nonfinite=True`` the norm the optimizer clips by
    (``optimizer.grad_norm``) and the finiteness it judges are therefore the global gradient's, on every rank.  The ranks agree
    on the clip coefficient to the last bit without exchanging it: the all-reduce leaves the same bits in every rank's buffer,
    and the norm's reduction is device-independent (its grid depends on the buffer's length alone and every partial sum has a
    fixed order, include/wavenet_hip.h), so identical buffers give identical coefficients and the weights cannot drift apart.

    Frozen parameters change nothing in what is exchanged: whole buckets, in which the ranges of frozen tensors
    travel as unspecified values nobody reads.  EVERY RANK MUST FREEZE THE SAME SET (nothing checks it): the optimizer of each
    rank updates the ranges its own model calls live."""

    def __init__(self, model, process_group=None, layers_per_bucket=None, exchange_when_alone=False):
        """``layers_per_bucket``: residual layers per gradient bucket = per weight-gradient launch group of wn_backward.
        Default (None): chosen by the size of the gradient.
          * small models (the BASELINE 64 / 256 model: 6.4 MB): ALL layers in one bucket, i.e. three buckets
            [post-net] [skip_1x1 + residual layers] [front + upsampling] (wn_bucket_range: with one layer bucket the skip tensors
            belong to it -- their gradients are made behind the chain, in the launch that also makes the res_1x1 gradients).
            Measured on MI355X at N = 1
            (profiles/r03/visit3_chain_dw_pipelined_lpb_chainpairdiff.txt): 10.42 ms per step with one layer bucket, 10.49 with
            two (15 layers each), 10.64 with three -- the weight-gradient contractions are most efficient as ONE layer-batched
            launch per tensor kind.  What a split would hide is the all-reduce of the 5.7 MB layer bucket, a latency-bound
            ring of ~0.1 ms over xGMI: splitting costs as much compute as it could hide, so it is not done; the post-net
            bucket travels under the whole backward chain either way.
          * large models (gradient above 32 MB; the recipe-size 512 / 256 model: 185 MB, ~2 - 3 ms of ring time against a
            131 ms step): groups of 10 layers, so that two thirds of the layer gradients travel under the rest of the chain;
            at that width the launch-group cost is below 0.5 % of the step."""
        self.model = model
        self.group = process_group
        self.eng = model.engine
        if layers_per_bucket:
            self.lpb = int(layers_per_bucket)
        else:
            big = 4 * int(self.eng.n_params) > 32 * 1024 * 1024
            self.lpb = min(10, int(self.eng.n_layers)) if big else int(self.eng.n_layers)
        self.ranges = self.eng.bucket_ranges(self.lpb)
        # what the buckets leave uncovered of [0, n_params) -- nothing, for every layout wn_bucket_range makes; a final micro-step
        # of an accumulation cycle would finish such a gap on the caller's stream
        edges = [0] + [v for r in sorted(self.ranges) for v in r] + [int(self.eng.n_params)]
        self._gaps = [(a, b) for a, b in zip(edges[0::2], edges[1::2]) if a < b]
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        # tests: run the bucket-event / side-stream / all-reduce branch with a single rank too (RCCL then executes, on this GPU)
        self.exchange_alone = bool(exchange_when_alone) and dist.is_initialized()
        self.cuda = self.eng.device.type == "cuda"
        if self.cuda:
            self.side = torch.cuda.Stream(device=self.eng.device)
            self.events = [torch.cuda.Event() for _ in self.ranges]
            for e in self.events:  # create the underlying hipEvent_t handles
                e.record(torch.cuda.current_stream(self.eng.device))
        else:
            self.side, self.events = None, None
        # opt-in measurement of the EXPOSED part of the exchange (bench.py's `comm` block): an event after the last backward
        # launch and one after the caller's stream has joined the side stream; their distance is what the all-reduces did NOT
        # hide under the backward kernels
        self.measure_exposed = False
        self._exposed = []

    @property
    def grad_scale(self):
        return 1.0 / self.world

    def _step(self, x, h, t, y, **kw):
        if y is not None:   # mixture-of-logistics head: the target is the waveform value, not the token
            return self.model.mol_loss_and_backward(x, h, y, **kw)
        return self.model.loss_and_backward(x, h, t, **kw)

    def loss_and_backward(self, x, h, t, t_start=None, y=None, grad_scale=None, lengths=None, micro_step=None,
                          teacher_logits=None, distill_alpha=0.5, distill_temperature=1.0, class_weights=None,
                          label_smoothing=0.0, position_weights=None, normalize="weights"):
        """forward + loss + backward with the bucketed all-reduce overlapped; returns the local
        mean loss (device tensor).  ``y`` (B, T) float selects the mixture-of-logistics loss.
        ``grad_scale``: this rank's share of the global minibatch (default 1/world = equal shards; pass
        B_local / B_global when the shards are uneven, so that the summed gradient is the global-batch mean).
        ``lengths``: this rank's padded shard of sequences of unequal length (``WaveNet.loss_and_backward``).  The local loss
        is then the mean over the rank's own N_local = sum_b max(lengths[b] - t_start, 0) loss positions, so the right share
        is ``grad_scale = N_local / N_global`` (N_global: the same count over every rank's shard): the summed gradient is the
        gradient of the mean over all N_global positions.  Ranks may run different T.

        ``micro_step=(i, A)``: gradient accumulation (``WaveNet.loss_and_backward``).  The all-reduce is linear, so the SUM over
        the A micro-batches is exchanged once: a non-final micro-step exchanges nothing (same ``layers_per_bucket`` launch
        structure, no events, no side-stream work; its ``grad_accumulate`` launch covers the whole buffer on the caller's stream);
        the final one keeps the overlap -- per bucket the side stream waits for the bucket's event, finishes the sum on the
        bucket's range and all-reduces it.  ``grad_scale`` is then this rank's share of the loss positions of the whole
        optimizer step, over all ranks and micro-steps (default 1 / (world * A): equal shards, equal micro-batches).

        ``teacher_logits`` / ``distill_alpha`` / ``distill_temperature``: knowledge distillation on this rank's shard, handed to
        ``WaveNet.loss_and_backward`` on every route (the gradient is exchanged as ever; softmax head only).

        ``class_weights`` / ``label_smoothing`` / ``position_weights`` / ``normalize``: the weighted cross-entropy on this rank's
        shard, handed to ``WaveNet.loss_and_backward`` likewise.  With the shares ``N_local / N_global`` as ``grad_scale``,
        ``normalize="positions"`` makes the pooled objective exact; ``"weights"`` gives the share-weighted mean of the ranks'
        weighted means, as torch DDP does."""
        kw = {} if lengths is None else {"lengths": lengths}
        if class_weights is not None or float(label_smoothing) != 0.0 or position_weights is not None or normalize != "weights":
            if y is not None:
                raise ValueError("the weighted cross-entropy is defined for the softmax head: its options cannot go with y")
            kw.update(class_weights=class_weights, label_smoothing=label_smoothing, position_weights=position_weights,
                      normalize=normalize)
        if teacher_logits is not None:
            if y is not None:
                raise ValueError("distillation is defined for the softmax head: teacher_logits cannot go with y")
            kw.update(teacher_logits=teacher_logits, distill_alpha=distill_alpha, distill_temperature=distill_temperature)
        if self.eng.begin_micro_step(micro_step) is not None:   # (checks the pair against the cycle; None: a plain call, A = 1 included)
            return self._micro_step(x, h, t, y, t_start, grad_scale, micro_step, kw)
        if self.world == 1 and not self.exchange_alone:   # same launch structure as N > 1 (weight gradients flushed per bucket), no exchange
            return self._step(x, h, t, y, t_start=t_start, layers_per_bucket=self.lpb, **kw)
        gscale = self.grad_scale if grad_scale is None else float(grad_scale)
        if not self.cuda:
            loss = self._step(x, h, t, y, t_start=t_start, grad_scale=gscale, **kw)
            flat = self.eng.grads()
            for lo, hi in self.ranges:
                dist.all_reduce(flat[lo:hi], group=self.group)
            return loss
        handles = [e.cuda_event for e in self.events]
        loss = self._step(x, h, t, y, t_start=t_start, grad_scale=gscale, events=handles,
                          layers_per_bucket=self.lpb, **kw)
        self._exchange()
        return loss

    def _exchange(self, finish=False):
        """The side-stream half of a step whose backward recorded the bucket events: per bucket wait for its event, (``finish``:
        add the accumulator into the bucket's range,) all-reduce the range; then the caller's stream joins."""
        flat = self.eng.grads()
        main = torch.cuda.current_stream(self.eng.device)
        pair = None
        if self.measure_exposed:
            pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            pair[0].record(main)     # behind the last backward launch
        with torch.cuda.stream(self.side):
            for (lo, hi), ev in zip(self.ranges, self.events):
                self.side.wait_event(ev)
                if finish:
                    self.eng.accumulate_grads(_ACCUM_FINISH, lo, hi)
                dist.all_reduce(flat[lo:hi], group=self.group)
        main.wait_stream(self.side)
        if finish:
            for lo, hi in self._gaps:   # (empty for every layout wn_bucket_range makes: the buckets tile the buffer)
                self.eng.accumulate_grads(_ACCUM_FINISH, lo, hi)
        if pair is not None:
            pair[1].record(main)     # the caller's stream has joined the exchange
            self._exposed.append(pair)

    def _micro_step(self, x, h, t, y, t_start, grad_scale, micro_step, kw):
        i, A = int(micro_step[0]), int(micro_step[1])
        gscale = 1.0 / (self.world * A) if grad_scale is None else float(grad_scale)
        alone = self.world == 1 and not self.exchange_alone
        if i != A - 1 or alone or not self.cuda:
            # whole-buffer accumulate launch behind the backward on the caller's stream (FINISH on the last micro-step), then,
            # on the last micro-step of the gloo path, the all-reduces of the sum
            lpb = {} if (not self.cuda and not alone) else {"layers_per_bucket": self.lpb}
            loss = self._step(x, h, t, y, t_start=t_start, grad_scale=gscale, micro_step=micro_step, **lpb, **kw)
            if i == A - 1 and not alone:
                flat = self.eng.grads()
                for lo, hi in self.ranges:
                    dist.all_reduce(flat[lo:hi], group=self.group)
            return loss
        handles = [e.cuda_event for e in self.events]
        loss = self._step(x, h, t, y, t_start=t_start, grad_scale=gscale, events=handles, layers_per_bucket=self.lpb,
                          micro_step=micro_step, _accumulate=False, **kw)
        self._exchange(finish=True)
        return loss

    def comm_report(self):
        """What the exchange looked like (after a synchronize): ranks and backend as torch.distributed reports them, bucket
        sizes, the RCCL channel cap in effect, and -- over the steps taken with ``measure_exposed`` -- the time the caller's
        stream waited for the side stream after its last backward launch (exposed exchange per step, ms)."""
        rep = {"world": self.world, "backend": dist.get_backend(self.group) if dist.is_initialized() else None,
               "buckets": len(self.ranges), "bucket_bytes": [4 * int(hi - lo) for lo, hi in self.ranges],
               "layers_per_bucket": self.lpb, "NCCL_MAX_NCHANNELS": os.environ.get("NCCL_MAX_NCHANNELS"),
               "exchange": "one in-place all-reduce per bucket on a side stream, released by the bucket's HIP event"
                           if (self.world > 1 or self.exchange_alone) else "none (one rank)"}
        if self._exposed:
            ms = [a.elapsed_time(b) for a, b in self._exposed]
            rep["exposed_ms_per_step"] = {"mean": sum(ms) / len(ms), "min": min(ms), "max": max(ms), "steps": len(ms)}
            self._exposed = []
        return rep
