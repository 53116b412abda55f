"""Fused training step of the hot loop (reference: selene/__init__.py:288-291) without Python in
the middle: one C-ABI call enqueues train forward + loss + backward on the current stream and
leaves the 14 gradients in ONE flat fp32 buffer (the buffer a multi-GPU run all-reduces).

`StepEngine` is what `bench.py` times and what `selene.Trainer` uses when its criterion is one of
the two losses `get_loss` can return; `model(x)` + `loss.backward()` (autograd path) computes the
same thing through separate forward/backward calls.
"""
import ctypes as C

import torch

from . import _lib


def sync_buffers(ctx, dev, bufs=None):
    """The fp64 exchange buffers of the sync-BN phases of `ctx` (one per phase; phases without an
    exchange get a placeholder).  Their sizes depend on the model's shape only: `bufs` from an
    earlier call are reused when they still fit."""
    lib, h = ctx.lib, ctx.handle
    need = [int(lib.explainn_sync_exchange_elems(h, i)) for i in range(1, _lib.SYNC_PHASES + 1)]
    if bufs is not None and all(b.numel() >= max(n, 1) for b, n in zip(bufs, need)):
        return bufs
    return [torch.zeros(max(n, 1), device=dev, dtype=torch.float64) for n in need]


def sync_run(ctx, args, bufs, phases):
    """Enqueue the sync-BN phases `phases` (explainn_sync_phase) with `args` on the current stream of
    the context's device; yields each exchange buffer the caller must sum over the ranks in place
    before resuming.  A phase reads the exchange of the last exchanging phase before it."""
    lib, h = ctx.lib, ctx.handle
    for phase in phases:
        prev = [q for q in range(1, phase) if int(lib.explainn_sync_exchange_elems(h, q)) > 0]
        has_out = int(lib.explainn_sync_exchange_elems(h, phase)) > 0
        xb = bufs[phase - 1]
        ctx.call("explainn_sync_phase", phase, args, bufs[prev[-1] - 1] if prev else None, xb if has_out else None)
        if has_out:
            yield xb


def rank_seed(step_no, rank):
    """Default dropout seed of a step: distinct per rank, so that shards do not share masks."""
    return (step_no * 0x9E3779B97F4A7C15 + (int(rank) << 40)) & 0xFFFFFFFFFFFFFFFF


def flat_grads(params, dev, zero=False):
    """One flat fp32 buffer for the gradients of `params` (explainn_grads order), its per-parameter
    views and the explainn_grads table pointing into it: (flat, views, gs)."""
    alloc = torch.zeros if zero else torch.empty
    flat = alloc(sum(p.numel() for p in params), device=dev, dtype=torch.float32)
    views, off = [], 0
    gs = _lib.Grads()
    for field, p in zip(_lib.GRAD_FIELDS, params):
        v = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
        views.append(v)
        setattr(gs, field, v.data_ptr())
    return flat, views, gs


class StepEngine:
    def __init__(self, model, max_batch, loss="binary"):
        self.model = model
        self.dev = model._device()
        self.loss_kind = _lib.LOSS_BCE_WITH_LOGITS if loss == "binary" else _lib.LOSS_MSE
        self.max_batch = max_batch
        self.ctx = model._context(max_batch, self.dev)
        self.params = list(model.parameters())
        self.flat_grad, self.views, self.gs = flat_grads(self.params, self.dev, zero=True)
        # a model bank (architectures.ExplaiNNBank): logits (B,G,T) and one loss per member
        self.logits = model._logits_empty(max_batch, self.dev)
        self.loss = torch.zeros(model._groups, device=self.dev, dtype=torch.float32)
        self.ps, self._keep = model._params_struct(self.dev)
        self.step_no = 0

    def refresh_params(self):
        """Call after parameters were re-assigned (not needed after in-place optimiser steps)."""
        self.ps, self._keep = self.model._params_struct(self.dev)

    def attach_grads(self):
        """Point every parameter's .grad at its slice of the flat buffer (for torch optimisers)."""
        for p, v in zip(self.params, self.views):
            p.grad = v

    @property
    def conv_grad_elements(self):
        """Leading elements of flat_grad that the last part of the backward writes (conv_w, conv_b,
        bn1_w, bn1_b): the `split` of parallel.GradAllReduce."""
        return sum(p.numel() for p in self.params[:4])

    def _front(self, x):
        """What step and sync_phases do before their launches: grow logits to the batch, re-resolve
        the context, prepare x and stage it.  Returns (x pointer, stream).
        The context is re-resolved every step: an eval forward with a larger batch in between
        (validation batches larger than the train batch, selene/__init__.py:334) makes the model
        replace its context by a bigger one, and the one cached here would be closed."""
        m = self.model
        B = x.shape[0]
        if B > self.max_batch:
            self.max_batch = B
            self.logits = self.model._logits_empty(B, self.dev)
        self.ctx = m._context(self.max_batch, self.dev)
        if not (torch.is_tensor(x) and x.dtype == torch.float32):
            x = m._prep_input(x, self.dev)
        stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        # the model's own validation schedule (architectures.ExplaiNN.validate_input): the first
        # steps read the flag before computing and route a soft batch to the dense kernels, as
        # forward() does; later steps enqueue without a host sync and the Trainer reads the sticky
        # flag periodically; dense_input=True goes straight to the dense kernels
        xp, _ = m._stage(self.ctx, x)
        return xp, stream

    def sync_phases(self, x, y, B_global, seed=None, freeze_top_n_filters=0, keep_mask=None, rank=0):
        """The sync-BN step as a generator: it enqueues phase after phase of
        explainn_sync_phase and yields each exchange buffer (fp64, on the device) that the caller
        must sum over the ranks in place before it resumes the generator.  When the generator is
        exhausted this rank holds the logits of its rows, the loss of the whole batch and the
        whole batch's 14 gradients in flat_grad (no gradient all-reduce follows).  x: this rank's
        B_local rows; B_global: the sequences of all ranks; keep_mask: this rank's rows of a
        (B, 100U) dropout keep-mask, or None for the built-in generator (seeded per `rank` unless
        `seed` is given)."""
        B = x.shape[0]
        if seed is None:
            self.step_no += 1
            seed = rank_seed(self.step_no, rank)
        m = self.model
        if m.dense_input:
            raise ValueError("sync-BN works on one-hot input or base codes, not dense_input")
        mask = None
        if keep_mask is not None:
            mask = keep_mask.to(device=self.dev, dtype=torch.uint8).contiguous()
        xp, _ = self._front(x)
        self._xbufs = sync_buffers(self.ctx, self.dev, getattr(self, "_xbufs", None))
        a = _lib.SyncArgs(x=xp, targets=y.data_ptr(), dlogits=None, dl_scale=1.0, B_local=B,
                          B_global=int(B_global), params=C.pointer(self.ps), grads=C.pointer(self.gs),
                          loss_kind=self.loss_kind, dropout_p=float(m.dropout_p), seed=seed,
                          keep_mask=mask.data_ptr() if mask is not None else None,
                          freeze_top_n_filters=int(freeze_top_n_filters), logits=self.logits.data_ptr(),
                          loss_out=self.loss.data_ptr())
        yield from sync_run(self.ctx, a, self._xbufs, range(1, _lib.SYNC_PHASES + 1))
        m._touched()
        m._rt.token += 1

    def step(self, x, y, seed=None, freeze_top_n_filters=0, grad_sync=None, global_batch=None):
        """x (B,4,L) fp32 one-hot -- or base codes (uint8 (B,L) / architectures.BaseCodes) -- and
        y (B,T) fp32, both resident on the device.  Enqueues one train-mode forward + loss +
        backward; returns (logits view, loss tensor) without syncing.  With grad_sync (a
        parallel.GradAllReduce over flat_grad) the step also averages the gradients across ranks:
        the all-reduce of the FC/head gradients is enqueued as soon as they are final and runs
        under the filter-bank backward (explainn_train_step_fc / _conv)."""
        B = x.shape[0]
        sync = getattr(self.model, "sync_bn", None)
        if sync is not None:
            # sync-BN (parallel.sync_batchnorm): full-batch statistics; every gradient comes out
            # global, so grad_sync must not average it again
            if grad_sync is not None:
                raise ValueError("sync-BN steps produce the whole batch's gradients: no grad_sync")
            Bg = sync.global_batch(B) if global_batch is None else int(global_batch)
            for xb in self.sync_phases(x, y, Bg, seed=seed, freeze_top_n_filters=freeze_top_n_filters,
                                       rank=sync.rank):
                sync.reduce(xb)
            return self.logits[:B], self.loss
        if seed is None:
            self.step_no += 1
            seed = rank_seed(self.step_no, 0)
        m = self.model
        xp, stream = self._front(x)
        if grad_sync is None:
            _lib.check(self.ctx.lib.explainn_train_step(
                self.ctx.handle, xp, y.data_ptr(), B, C.byref(self.ps), C.byref(self.gs),
                self.loss_kind, float(m.dropout_p), C.c_uint64(seed), int(freeze_top_n_filters),
                self.logits.data_ptr(), self.loss.data_ptr(), stream))
        else:
            _lib.check(self.ctx.lib.explainn_train_step_fc(
                self.ctx.handle, xp, y.data_ptr(), B, C.byref(self.ps), C.byref(self.gs),
                self.loss_kind, float(m.dropout_p), C.c_uint64(seed), self.logits.data_ptr(),
                self.loss.data_ptr(), stream))
            work = grad_sync.start_tail()
            _lib.check(self.ctx.lib.explainn_train_step_conv(
                self.ctx.handle, B, C.byref(self.ps), C.byref(self.gs), int(freeze_top_n_filters),
                stream))
            grad_sync.finish(work)
        m._touched()
        m._rt.token += 1
        return self.logits[:B], self.loss
