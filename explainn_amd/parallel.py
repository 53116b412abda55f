"""Data-parallel glue: one process per GPU, minibatches sharded across ranks, ONE collective per
step -- an all-reduce (average) of the flat fp32 gradient buffer over RCCL/xGMI.

Opt-in sync-BN (`sync_batchnorm`): every BatchNorm takes the statistics of
the whole batch; the step then exchanges six small buffers of sums between its phases and no
gradient all-reduce follows.  A reducer sums a tensor in place across ranks: `ProcessGroupReducer`
over torch.distributed, `VirtualRanks` for R shards driven inside one process on one device.

The reference has no multi-device path at all (selene/__init__.py:98-100 leaves data_parallel
commented out); semantics here are those `torch DDP` would give the reference module: per-shard
BatchNorm statistics, averaged gradients, rank-0 parameters broadcast at start.
"""
import torch
import torch.distributed as dist


def world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def rank():
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def shard_bounds(n_items, world_size, r):
    """Contiguous shard [lo, hi) of rank r; the first n_items % world_size ranks get one more."""
    base, extra = divmod(n_items, world_size)
    lo = r * base + min(r, extra)
    return lo, lo + base + (1 if r < extra else 0)


def shard_batch(x, y):
    lo, hi = shard_bounds(x.shape[0], world(), rank())
    return x[lo:hi], y[lo:hi]


def broadcast_parameters(model, src=0):
    """Make every rank start from rank `src`'s parameters and BatchNorm buffers."""
    if world() == 1:
        return
    tensors = list(model.parameters()) + list(model.buffers())
    for t in tensors:
        dist.broadcast(t.data, src)
    # the broadcast wrote through `.data`, which torch's version counters do not see: tell the
    # model (cached eval tables, explainn_params.version) that the values moved
    torch.autograd.graph.increment_version(tensors)
    if hasattr(model, "invalidate"):
        model.invalidate()


def average_gradients(flat):
    """All-reduce (average) of a flat gradient buffer: the `grad_sync` callable of the autograd
    path (ExplaiNN._launch_backward calls it with the buffer all 14 gradients are views of)."""
    if world() > 1:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        flat.div_(world())
    return flat


class GradAllReduce:
    """Averages one flat gradient buffer across ranks: a single collective per step.  At C2 the
    buffer is 3.7 MB; RCCL picks its own algorithm."""

    def __init__(self, flat, split=0, force=False):
        """split: number of leading elements (conv_w, conv_b, bn1_w, bn1_b in explainn_grads order)
        that only the last part of the backward produces; everything behind it is final earlier and
        can be reduced while that part still runs (`start_tail` / `finish`, used by StepEngine)."""
        self.flat = flat
        self.split = int(split)
        self.n = world()
        # force: issue the collectives even in a one-rank group (they are identities there); lets a
        # single-GPU test drive the asynchronous RCCL path
        self.single = self.n == 1 and not force
        self.native_avg = False
        if not self.single and dist.get_backend() == "nccl":
            # ReduceOp.AVG saves the scaling pass; probe it once (all ranks take the same branch)
            try:
                probe = torch.ones(1, device=flat.device)
                dist.all_reduce(probe, op=dist.ReduceOp.AVG)
                self.native_avg = abs(float(probe.item()) - 1.0) < 1e-6
            except Exception:
                self.native_avg = False

    def _reduce(self, t, async_op=False):
        op = dist.ReduceOp.AVG if self.native_avg else dist.ReduceOp.SUM
        return dist.all_reduce(t, op=op, async_op=async_op)

    def start_tail(self):
        """Enqueue the all-reduce of flat[split:] (the per-unit FC / head gradients) without making
        the launch stream wait for it; returns the work handle for `finish`."""
        if self.single or self.split <= 0 or self.split >= self.flat.numel():
            return None
        return self._reduce(self.flat[self.split:], async_op=True)

    def finish(self, work):
        """All-reduce what `start_tail` left (everything if it returned None), then make the launch
        stream wait for both."""
        if self.single:
            return self.flat
        if work is None:
            return self()
        # the head slice (conv_w, conv_b, bn1_w, bn1_b) goes to RCCL's stream as well: enqueued there
        # behind an event of the launch stream, so the tail reduce still in flight and this one
        # queue up on RCCL's side while the launch stream only waits once, for both
        head = self._reduce(self.flat[:self.split], async_op=True)
        work.wait()
        head.wait()
        if not self.native_avg:
            self.flat.div_(self.n)
        return self.flat

    def __call__(self, flat=None):
        t = self.flat if flat is None else flat
        if self.single:
            return t
        if self.native_avg:
            dist.all_reduce(t, op=dist.ReduceOp.AVG)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            t.div_(self.n)
        return t


class ProcessGroupReducer:
    """reduce(t): in-place SUM of t across the ranks of the default process group.  Backends that
    do not take device tensors (gloo) are staged through the host."""

    def __init__(self, group=None):
        self.group = group

    @property
    def rank(self):
        return rank()

    def _staged(self, t):
        return t.is_cuda and dist.get_backend(self.group) == "gloo"

    def reduce(self, t):
        if world() == 1:
            return t
        if self._staged(t):
            h = t.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group)
            t.copy_(h)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def global_batch(self, b_local):
        """Sequences of all ranks in this step: one small collective and a host read.  A caller
        that knows the global batch (Trainer, bench-style loops) passes it to StepEngine.step /
        the forward instead; it is not cached by B_local, because an uneven last batch can change
        the other ranks' shards while this rank's stays the same size."""
        if world() == 1:
            return int(b_local)
        n = torch.tensor([int(b_local)], dtype=torch.int64)
        if dist.get_backend(self.group) != "gloo":
            n = n.cuda()
        dist.all_reduce(n, op=dist.ReduceOp.SUM, group=self.group)
        return int(n.item())


class VirtualRanks:
    """R data-parallel ranks inside one process: rank r is a model replica with its own StepEngine
    (its own context and BatchNorm buffers).  `step` drives the R sync-BN steps phase by phase and
    sums every exchange over the ranks in rank order, so all ranks receive identical bits -- what
    R devices would compute, on one.  It is the driver of its ranks, not a reducer: one rank cannot
    sum on its own, so it is not what sync_batchnorm takes (the replicas' models stay per-shard;
    `step` calls their engines' sync_phases directly)."""

    def __init__(self, engines):
        self.engines = list(engines)

    @property
    def size(self):
        return len(self.engines)

    def step(self, xs, ys, keep_masks=None, seeds=None, freeze_top_n_filters=0):
        """xs, ys: per-rank shards.  Returns per-rank (logits, loss) like StepEngine.step."""
        R = self.size
        if len(xs) != R or len(ys) != R:
            raise ValueError("one shard of x and y per virtual rank")
        Bg = sum(int(x.shape[0]) for x in xs)
        gens = [e.sync_phases(xs[r], ys[r], Bg, rank=r,
                              seed=None if seeds is None else seeds[r],
                              freeze_top_n_filters=freeze_top_n_filters,
                              keep_mask=None if keep_masks is None else keep_masks[r])
                for r, e in enumerate(self.engines)]
        while True:
            bufs = [next(g, None) for g in gens]
            if all(b is None for b in bufs):
                break
            if any(b is None for b in bufs):
                raise RuntimeError("virtual ranks out of step")
            tot = bufs[0].clone()
            for b in bufs[1:]:
                tot += b
            for b in bufs:
                b.copy_(tot)
        return [(e.logits[:int(x.shape[0])], e.loss) for e, x in zip(self.engines, xs)]


def sync_batchnorm(model, reducer):
    """Switch `model` to full-batch BatchNorm statistics across the ranks `reducer` spans (the
    counterpart of torch's convert_sync_batchnorm); reducer None switches back to per-shard
    statistics.  StepEngine.step then runs the phased step and leaves the whole batch's gradients
    on every rank -- do not average them again (no grad_sync)."""
    if reducer is not None and not all(hasattr(reducer, a) for a in ("reduce", "global_batch", "rank")):
        raise TypeError("sync_batchnorm needs a reducer with reduce(tensor), global_batch(b) and rank "
                        "(ProcessGroupReducer); VirtualRanks drives its replicas itself (VirtualRanks.step)")
    model.sync_bn = reducer
    return model
