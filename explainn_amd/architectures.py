"""Drop-in `ExplaiNN` nn.Module whose forward/backward run as hand-written gfx950 kernels.

Mirrors the reference's module surface for this path (reference: explainn/architectures/__init__.py):
  * constructor `ExplaiNN(cnn_units, kernel_size, sequence_length, n_features=1, weights_file=None)`
    and `_options`                                                         (:44-67)
  * `state_dict()` keys/shapes `linears.{0,1,6,7,10,11}.*`, `final.*`      (:72-104)
  * `forward(x)`: x (B,4,L) fp32 one-hot -> logits (B,T); train mode uses batch statistics,
    updates the BatchNorm buffers and applies Dropout(0.3)                 (:109-114)
  * `model.linears[0].weight`, `model.linears(x_rep)`, `model.linears[:3](x_rep)`,
    `model.final(outs)` as test.py:148-160 / train.py:318-324 / selene/__init__.py:257 use them
  * `get_loss`, `get_metrics`, `get_optimizer`                             (:446-464)

The compute is in libexplainn_hip.so (include/explainn_hip.h); PyTorch only owns the device
memory, the stream and autograd bookkeeping.  There is no CPU or eager fallback: a model that is
not on a HIP device raises.
"""
import contextlib
import copy
import ctypes as C
import math
import weakref
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .engine import flat_grads, rank_seed, sync_buffers, sync_run

FC_HIDDEN = 100
POOL = 7
DROPOUT_P = 0.3


# ----------------------------------------------------------------------------------------------
# parameter holders (positions 0,1,6,7,10,11 of `linears`; the other positions hold no state)
# ----------------------------------------------------------------------------------------------
def _uniform_fan_in_(weight, bias, fan_in):
    """torch's default Conv1d/Linear init: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for both."""
    bound = 1.0 / math.sqrt(fan_in) if fan_in > 0 else 0.0
    with torch.no_grad():
        weight.uniform_(-bound, bound)
        bias.uniform_(-bound, bound)


class _GroupedTaps(nn.Module):
    """weight/bias of a grouped Conv1d; holds state only (the kernels do the math)."""

    def __init__(self, out_channels, in_per_group, kernel_size):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_per_group, kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels))
        _uniform_fan_in_(self.weight, self.bias, in_per_group * kernel_size)

    def forward(self, *a, **k):
        raise RuntimeError("sub-layers are fused; call model(x), model.linears(x_rep) or "
                           "model.linears[:3](x_rep)")


class _BatchStats(nn.Module):
    """BatchNorm1d state: affine parameters and running statistics."""

    def __init__(self, channels):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(channels))
        self.bias = nn.Parameter(torch.zeros(channels))
        self.register_buffer("running_mean", torch.zeros(channels))
        self.register_buffer("running_var", torch.ones(channels))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    forward = _GroupedTaps.forward


class _Fused(nn.Module):
    """Stateless stage (exp, max-pool, flatten, ReLU, dropout) -- fused into the kernels."""

    def __init__(self, what):
        super().__init__()
        self.what = what

    def extra_repr(self):
        return self.what

    forward = _GroupedTaps.forward


class _UnitPrefix:
    """`model.linears[:3]` -- conv + BatchNorm + exp per position (test.py:159-160)."""

    def __init__(self, owner):
        self._owner = owner

    def __call__(self, x_rep):
        return self._owner._unit_activations(x_rep)


class _UnitStack(nn.Sequential):
    """The `linears` container: real parameters at the reference's indices, fused forward."""

    def _bind(self, owner):
        self.__dict__["_owner_ref"] = weakref.ref(owner)

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_owner_ref", None)           # re-bound by the owner's __setstate__/__deepcopy__
        return state

    def _owner(self):
        owner = self.__dict__["_owner_ref"]()
        if owner is None:
            raise RuntimeError("owning ExplaiNN module is gone")
        return owner

    def forward(self, x_rep):
        return self._owner()._unit_outputs(x_rep)

    def __getitem__(self, idx):
        if isinstance(idx, slice):
            if idx == slice(None, 3, None) or idx == slice(0, 3, None):
                return _UnitPrefix(self._owner())
            raise NotImplementedError("only linears[:3] (conv+BN+exp) is exposed as a sub-stack")
        return super().__getitem__(idx)


class BaseCodes:
    """A batch handed over as base codes instead of an fp32 one-hot: `codes` is a
    (B,L) uint8 tensor on the model's device, 0..3 = A,C,G,T, 4 = N (sequence.encode_codes_many);
    reverse_complement=True makes the kernel read it as its reverse complement, so the strand
    augmentation of train.py:275-278 / predict.py:78-79 needs no second copy.  Accepted wherever
    the model takes `x`; a bare uint8 (B,L) tensor means BaseCodes(codes, False)."""

    def __init__(self, codes, reverse_complement=False):
        self.codes = codes
        self.reverse_complement = bool(reverse_complement)

    @property
    def shape(self):
        return self.codes.shape


def _check_codes(codes, dev, subject):
    """A device-resident sequence of base codes as the context reads it; `subject` opens the message."""
    if not torch.is_tensor(codes) or codes.dtype != torch.uint8 or codes.dim() != 1 or not codes.is_contiguous():
        raise RuntimeError("%s a contiguous 1-D uint8 tensor of base codes" % subject)
    if codes.device != dev:
        raise RuntimeError("input is on %s but the model is on %s" % (codes.device, dev))


class _SequenceRows:
    """A batch whose rows the context cuts out of ONE device-resident sequence of base codes (1-D uint8)
    itself, `sub_batch` of them per device pass."""

    def __init__(self, codes, n_rows, reverse_complement, sub_batch):
        self.codes, self.n_rows = codes, int(n_rows)
        self.reverse_complement = bool(reverse_complement)
        self.sub_batch = max(1, min(int(sub_batch), self.n_rows))

    @property
    def shape(self):
        """(sequences per device pass, L): what _front sizes the context by."""
        return (self.sub_batch, None)


class SequenceWindows(_SequenceRows):
    """The windows codes[start + i*stride : ... + L], i < n_windows, as ExplaiNN._launch_scan takes them
    (explainn_scan)."""

    def __init__(self, codes, start, n_windows, stride, reverse_complement=False, sub_batch=4096):
        super().__init__(codes, n_windows, reverse_complement, sub_batch)
        self.start, self.n_windows, self.stride = int(start), self.n_rows, int(stride)

    def check(self, dev):
        _check_codes(self.codes, dev, "a scan takes")


class EditedWindows(_SequenceRows):
    """Windows at arbitrary starts, each with at most one edit spliced in, as ExplaiNN._launch_score_edits
    takes them (explainn_score_edits, include/explainn_hip.h has the row definition).  All tables are
    contiguous tensors on the codes' device: row_start int64 (rows,), row_edit int32 (rows,) with -1 = no
    edit; pos int64, ref_len / alt_len / alt_off int32 (edits,); alt uint8, the pool of alt base codes."""

    _TABLES = (("row_start", torch.int64), ("row_edit", torch.int32), ("pos", torch.int64),
               ("ref_len", torch.int32), ("alt_len", torch.int32), ("alt_off", torch.int32), ("alt", torch.uint8))
    # the struct of these tables, its count fields (each the length of a table), the tables with one entry per row
    _STRUCT = (_lib.Edits, (("n_edits", "pos"), ("alt_bytes", "alt")), ("row_start", "row_edit"))

    def __init__(self, codes, row_start, row_edit, pos, ref_len, alt_len, alt_off, alt,
                 reverse_complement=False, sub_batch=4096):
        self._init_tables(codes, (row_start, row_edit, pos, ref_len, alt_len, alt_off, alt), reverse_complement,
                          sub_batch)

    def _init_tables(self, codes, tables, reverse_complement, sub_batch):
        for (name, _), t in zip(self._TABLES, tables):
            setattr(self, name, t)
        _SequenceRows.__init__(self, codes, tables[0].numel(), reverse_complement, sub_batch)

    def check(self, dev):
        _check_codes(self.codes, dev, "edited windows take")
        for name, dt in self._TABLES:
            t = getattr(self, name)
            if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.device != dev:
                raise RuntimeError("%s must be a contiguous 1-D %s tensor on %s" % (name, dt, dev))
        per_row = self._STRUCT[2]
        if any(getattr(self, name).numel() != self.n_rows for name in per_row):
            raise RuntimeError("%s and %s must have one entry per row" % (", ".join(per_row[:-1]), per_row[-1]))
        if not self.pos.numel() == self.ref_len.numel() == self.alt_len.numel() == self.alt_off.numel():
            raise RuntimeError("pos, ref_len, alt_len and alt_off must have one entry per edit")

    def struct(self):
        """The explainn_edits / explainn_haplotypes of these tables (valid while this object lives)."""
        cls, counts, _ = self._STRUCT
        st = cls()
        for name, _ in self._TABLES:
            t = getattr(self, name)
            setattr(st, name, t.data_ptr() if t.numel() else None)
        for field, name in counts:
            setattr(st, field, getattr(self, name).numel())
        return st


class HaplotypeWindows(EditedWindows):
    """Windows at arbitrary starts, each carrying a RUN of edits, as ExplaiNN._launch_score_haplotypes
    takes them (explainn_score_haplotypes, include/explainn_hip.h has the run algebra and the ordering
    rule).  Contiguous tensors on the codes' device: row_start int64, row_first int64, row_count int32
    (rows,); edit_index int32, the rows' runs as indices into the edit table; pos int64, ref_len / alt_len /
    alt_off int32 (edits,); alt uint8.  Row b carries the edits
    edit_index[row_first[b] : row_first[b] + row_count[b]]."""

    _TABLES = (("row_start", torch.int64), ("row_first", torch.int64), ("row_count", torch.int32),
               ("edit_index", torch.int32), ("pos", torch.int64), ("ref_len", torch.int32),
               ("alt_len", torch.int32), ("alt_off", torch.int32), ("alt", torch.uint8))
    _STRUCT = (_lib.Haplotypes, (("n_index", "edit_index"), ("n_edits", "pos"), ("alt_bytes", "alt")),
               ("row_start", "row_first", "row_count"))

    def __init__(self, codes, row_start, row_first, row_count, edit_index, pos, ref_len, alt_len, alt_off, alt,
                 reverse_complement=False, sub_batch=4096):
        self._init_tables(codes, (row_start, row_first, row_count, edit_index, pos, ref_len, alt_len, alt_off, alt),
                          reverse_complement, sub_batch)


VALIDATE_EVERY = 64      # deferred input validation: the sticky device flag is read every this many calls

# How ExplaiNN._stage treats an fp32 batch (base codes are always staged):
SCHEDULED = "scheduled"            # validate_input's schedule decides whether the flag is read first
VALIDATE_FIRST = "validate-first"  # read it before computing; a soft batch takes the dense kernels
ONEHOT_ONLY = "one-hot only"       # read it before computing; dense_input or a soft batch raises

# attributes resolved against one handle's own modules: not copied, pickled or shared by a replica
_PER_HANDLE = ("_slots", "_ps_cache", "_vkey", "_bufs")


class _Runtime:
    """Per-model device context; never copied or pickled with the module."""

    def __init__(self):
        self.ctx = None
        self.token = 0
        self.pending = None
        self.sync = None         # sync-BN forward awaiting its backward (_launch_train_sync)
        self.sync_bufs = None    # its exchange buffers
        self.x_keep = None
        self.calls = 0           # forwards since the model was built (input validation schedule)
        self.soft_seen = False   # a validating call met a batch that was not one-hot
        self.cache_depth = 0     # nesting depth of eval_cache() scopes
        self.replica = None      # eval_replica(): second handle on the same tensors, own context
        self.side_stream = None  # the stream predict() runs the replica on

    def __deepcopy__(self, memo):
        return _Runtime()

    def __getstate__(self):
        return {}

    def __setstate__(self, state):
        self.__init__()


class _TrainStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, *params):
        ctx.model = model
        ctx.x_dtype = x.dtype if torch.is_tensor(x) else None
        # x.grad wanted: validate this batch before computing, so that soft input takes the dense
        # kernels (and its gradient is the gradient at that x)
        want_dx = torch.is_tensor(x) and x.requires_grad
        logits, ctx.token = model._launch_train(x, VALIDATE_FIRST if want_dx else SCHEDULED)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        if ctx.needs_input_grad[1]:
            grads, dx = ctx.model._launch_backward(dlogits, ctx.token, want_dx=True)
            return (None, dx.to(ctx.x_dtype)) + tuple(grads)
        grads = ctx.model._launch_backward(dlogits, ctx.token)
        return (None, None) + tuple(grads)


class _EvalInputGrad(torch.autograd.Function):
    """Eval-mode forward whose logits carry a grad_fn back to x (saliency, gradient x input,
    Integrated Gradients): the gradient flows to x only -- an eval forward gives no parameter
    gradients, as before."""

    @staticmethod
    def forward(ctx, model, x):
        ctx.model = model
        ctx.x_dtype = x.dtype
        logits, ctx.token = model._launch_eval_keep(x)
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits):
        return None, ctx.model._launch_input_grad(dlogits, ctx.token).to(ctx.x_dtype)


class _Model(nn.Module):

    def load_weights(self, weight_file):
        """architectures/__init__.py:27-39: positional remap of a saved tensor list onto this
        module's keys.  Accepts both the (100U,n,1)/(U,100,1) layout of this class's own
        state_dict and the squeezed (100U,n)/(U,100) layout of the older Linear-based variant."""
        sd = torch.load(weight_file, map_location="cpu", weights_only=True)
        own = self.state_dict()
        keys = list(own.keys())
        remapped = OrderedDict()
        for key, v in zip(keys, sd.values()):
            if v.dim() == own[key].dim() - 1:
                v = v.unsqueeze(-1)
            elif v.dim() == own[key].dim() + 1 and v.shape[-1] == 1:
                v = v.squeeze(-1)
            remapped[key] = v
        self.load_state_dict(remapped)


class ExplaiNN(_Model):
    """ExplaiNN: explainable neural networks (MI355X-native forward/backward)."""

    def __init__(self, cnn_units, kernel_size, sequence_length, n_features=1, weights_file=None):
        super().__init__()
        self._options = {
            "cnn_units": cnn_units,
            "kernel_size": kernel_size,
            "sequence_length": sequence_length,
            "n_features": n_features,
            "weights_file": weights_file,
        }
        if cnn_units < 1 or n_features < 1 or kernel_size < 1:
            # torch's Conv1d/Linear constructors reject these in the reference
            raise ValueError("cnn_units, kernel_size and n_features must be positive")
        n = int(math.floor((sequence_length - kernel_size + 1) / float(POOL)))
        if n < 1:
            raise ValueError("sequence_length too short for kernel_size and MaxPool1d(7, 7)")
        self._n = n
        U = cnn_units
        self.linears = _UnitStack(
            _GroupedTaps(U, 4, kernel_size),                 # 0  Conv1d(4U->U, k, groups=U)
            _BatchStats(U),                                  # 1  BatchNorm1d(U)
            _Fused("exp"),                                   # 2
            _Fused("max_pool1d(7, 7)"),                      # 3
            _Fused("flatten"),                               # 4
            _Fused("unsqueeze(-1)"),                         # 5
            _GroupedTaps(FC_HIDDEN * U, n, 1),               # 6  per-unit Linear(n->100)
            _BatchStats(FC_HIDDEN * U),                      # 7  BatchNorm1d(100U)
            _Fused("relu"),                                  # 8
            _Fused("dropout(p=%g)" % DROPOUT_P),             # 9
            _GroupedTaps(U, FC_HIDDEN, 1),                   # 10 per-unit Linear(100->1)
            _BatchStats(U),                                  # 11 BatchNorm1d(U)
            _Fused("relu"),                                  # 12
            _Fused("flatten"),                               # 13
        )
        self.linears._bind(self)
        self.final = nn.Linear(U, n_features)
        self.dropout_p = DROPOUT_P
        # Input validation (is every column of x one-hot or all-zero?) happens on the device while
        # the batch is packed and raises a sticky flag.  True: the first two forwards read the flag
        # before computing (so that a soft batch is routed to the dense kernels), later ones
        # enqueue and return without touching the host; the flag is then read every
        # VALIDATE_EVERY-th call, by check_input(), and at the end of predict() / a validation pass.
        # "always": every call validates before computing (one host sync per forward).
        # False: never.
        self.validate_input = True
        # None: a batch that fails validation takes the dense kernels (the reference accepts any
        # float input); True: always dense; False: a batch that is not one-hot is an error
        self.dense_input = None
        self.grad_sync = None          # optional callable(flat_grad_tensor): multi-GPU all-reduce
        self.sync_bn = None            # parallel.sync_batchnorm: a reducer -> full-batch BatchNorm statistics
        # rows [0:n) of the filter gradient are zeroed inside the backward kernel (what the hook of
        # selene/__init__.py:254-257, 509-515 does to the reference's gradient)
        self.freeze_top_n_filters = 0
        self._rt = _Runtime()
        if weights_file is not None:
            self.load_weights(weights_file)

    # -- module protocol ------------------------------------------------------------------
    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for key, val in self.__dict__.items():
            if key in _PER_HANDLE:
                continue
            new.__dict__[key] = _Runtime() if key == "_rt" else copy.deepcopy(val, memo)
        new.linears._bind(new)
        return new

    def __getstate__(self):
        state = self.__dict__.copy()
        for key in _PER_HANDLE:             # ctypes tables: rebuilt on demand
            state.pop(key, None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__["_rt"] = _Runtime()
        for key in _PER_HANDLE:
            self.__dict__.pop(key, None)
        self.linears._bind(self)

    def eval_replica(self):
        """A second handle on the SAME parameters and buffers (the very tensor objects) with its own
        device context, for eval-mode forwards that overlap this model's on another stream: a
        forward is four dependent launches, and two independent batches in flight fill the gaps
        between them (batch 1024: 18 -> 25 M sequences/s).  predict() runs the two strands of a chunk
        this way.  Forward only; the replica follows this model's mode and input settings at the
        time of the call."""
        r = self._rt.replica
        if r is None:
            r = self.__class__.__new__(self.__class__)
            for key, val in self.__dict__.items():
                if key in _PER_HANDLE or key == "_pver":
                    continue
                r.__dict__[key] = val
            r.__dict__["_rt"] = _Runtime()
            self._rt.replica = r
        r.__dict__["training"] = self.training
        r.__dict__["validate_input"] = self.validate_input
        r.__dict__["dense_input"] = self.dense_input
        return r

    # -- plumbing -------------------------------------------------------------------------
    def _device(self):
        dev = self.final.weight.device
        if dev.type != "cuda":
            raise RuntimeError(
                "explainn_amd.ExplaiNN runs only on a HIP device (model is on %s): call "
                ".cuda()/.to('cuda'). There is no CPU fallback." % dev)
        return dev

    # What a model bank (ExplaiNNBank below) answers differently: the units the kernels run on, the
    # members of the context and the shape of the logits.
    _groups = 1

    def _units(self):
        return self._options["cnn_units"]

    def _logits_empty(self, B, dev):
        return torch.empty(B, self._options["n_features"], device=dev, dtype=torch.float32)

    def _context(self, B, dev):
        o = self._options
        geom = (o["cnn_units"], o["kernel_size"], o["sequence_length"], o["n_features"])
        ctx = self._rt.ctx
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        if ctx is None or ctx.geom != geom or ctx.device != index or ctx.max_batch < B:
            if ctx is not None:
                torch.cuda.synchronize(dev)
                ctx.close()
            cap = max(B, ctx.max_batch if ctx is not None and ctx.geom == geom else 0)
            self._rt.ctx = _lib.Context(*geom, max_batch=cap, device=index, groups=self._groups)
        return self._rt.ctx

    def __setattr__(self, name, value):
        if name in ("final", "linears"):
            self.__dict__.pop("_slots", None)          # sub-module replaced: re-resolve the slots
        super().__setattr__(name, value)

    def _param_slots(self):
        """(C field, the owning module's parameter/buffer dict, name, dtype) for the 23 tensors of
        explainn_params, resolved once: the per-call check is then 23 dict lookups instead of
        walking named_parameters() or going through nn.Module.__getattr__."""
        slots = self.__dict__.get("_slots")
        if slots is None:
            slots = []
            for field in _lib.PARAM_FIELDS:
                path = _lib.PARAM_KEYS[field].split(".")
                mod = self
                for part in path[:-1]:
                    mod = mod[int(part)] if part.isdigit() else getattr(mod, part)
                store = mod._parameters if path[-1] in mod._parameters else mod._buffers
                slots.append((field, store, path[-1],
                              torch.int64 if field.endswith("nbt") else torch.float32))
            self.__dict__["_slots"] = slots
            self.__dict__.pop("_ps_cache", None)
        return slots

    def _params_struct(self, dev):
        """The explainn_params table (+ the tensors it points into, kept alive with it).  Cached
        until a parameter object is replaced (train.py:324 re-assigns the filter bank) or its
        storage moves (`.cuda()`, `.data = ...`); in-place optimiser updates keep it valid."""
        slots = self._param_slots()
        cache = self.__dict__.get("_ps_cache")
        if cache is not None and cache[0] == dev:
            _, ps, keep, ptrs = cache
            for (field, store, attr, want), t, ptr in zip(slots, keep, ptrs):
                cur = store[attr]
                if cur is not t or cur.data_ptr() != ptr:
                    break
            else:
                self._stamp_version(ps, keep)
                return ps, keep
        ps = _lib.Params()
        keep, ptrs = [], []
        for field, store, attr, want in slots:
            t = store[attr]
            if t.device != dev or t.dtype != want:
                raise RuntimeError("parameter %s must be %s on %s (is %s on %s)" % (
                    _lib.PARAM_KEYS[field], want, dev, t.dtype, t.device))
            if not t.is_contiguous():
                raise RuntimeError("parameter %s must be contiguous" % _lib.PARAM_KEYS[field])
            keep.append(t)
            ptrs.append(t.data_ptr())
            setattr(ps, field, ptrs[-1])
        self.__dict__["_ps_cache"] = (dev, ps, keep, ptrs)
        self.__dict__["_bufs"] = [t for (field, _, _, _), t in zip(slots, keep)
                                  if field.endswith(("_rm", "_rv", "_nbt"))]
        self.__dict__.pop("_vkey", None)
        self._stamp_version(ps, keep)
        return ps, keep

    def _stamp_version(self, ps, keep):
        """explainn_params.version: 0 ("unknown": the eval entry points rebuild their folded
        tables on every call) unless an eval_cache() scope is open; inside one, a counter that
        moves whenever any of the 23 tensors changed value as far as torch can tell (its per-tensor
        version counters; this package's own kernels, which write through raw pointers, bump
        them explicitly -- _touched()).  Writes through `.data` do NOT move torch's counters
        (`p.data.clamp_(0)`, selene/__init__.py:294), which is why caching is opt-in and scoped:
        the scope's owner promises not to do that inside it, or calls invalidate()."""
        if self._rt.cache_depth <= 0:
            ps.version = 0
            return
        vkey = tuple(t._version for t in keep)
        if vkey != self.__dict__.get("_vkey"):
            self.__dict__["_vkey"] = vkey
            self.__dict__["_pver"] = self.__dict__.get("_pver", 0) + 1
        ps.version = self.__dict__["_pver"]

    def invalidate(self):
        """Forget the cached eval-mode tables (after writing parameters or buffers through `.data`
        or raw pointers inside an eval_cache() scope)."""
        self.__dict__["_pver"] = self.__dict__.get("_pver", 0) + 1
        self.__dict__.pop("_vkey", None)

    @contextlib.contextmanager
    def eval_cache(self):
        """Scope in which eval-mode forwards reuse the folded tables (filter LUTs, BatchNorm folds,
        FC1 fragments) of the previous call instead of rebuilding them per batch -- predict(), a
        validation pass and the filter export open one around their loops.  Contract: inside the
        scope parameters and buffers change only through torch ops that bump tensor versions
        (optimiser steps, in-place ops on the tensor itself, load_state_dict, re-assignment) or
        through this package's kernels; after a `.data` write call invalidate()."""
        self._rt.cache_depth += 1
        if self._rt.cache_depth == 1:
            self.invalidate()            # whatever happened outside the scope is unknown
        try:
            yield self
        finally:
            self._rt.cache_depth -= 1

    def _touched(self):
        """The train-mode kernels updated the BatchNorm buffers in place (as torch does)."""
        torch.autograd.graph.increment_version(self.__dict__.get("_bufs") or list(self.buffers()))

    def _prep_input(self, x, dev):
        o = self._options
        if isinstance(x, BaseCodes) or (torch.is_tensor(x) and x.dtype == torch.uint8 and x.dim() == 2):
            bc = x if isinstance(x, BaseCodes) else BaseCodes(x)
            c = bc.codes
            if not torch.is_tensor(c) or c.dtype != torch.uint8 or c.dim() != 2 or \
                    c.shape[1] != o["sequence_length"]:
                raise RuntimeError("base codes must be a uint8 tensor of shape (B, %d)" % o["sequence_length"])
            if c.device != dev:
                raise RuntimeError("input is on %s but the model is on %s" % (c.device, dev))
            return BaseCodes(c.detach().contiguous(), bc.reverse_complement)
        if x.dim() != 3 or x.shape[1] != 4 or x.shape[2] != o["sequence_length"]:
            raise RuntimeError("expected input of shape (B, 4, %d), got %s" % (
                o["sequence_length"], tuple(x.shape)))
        if x.device != dev:
            raise RuntimeError("input is on %s but the model is on %s" % (x.device, dev))
        return x.detach().to(torch.float32).contiguous()

    def _validate_now(self):
        """Does THIS forward read the validation flag before computing?  (validate_input above.)"""
        v = self.validate_input
        if not v:
            return False
        # a model that has met a soft batch once keeps validating (and routing) per call
        return v == "always" or self._rt.soft_seen or self._rt.calls <= 2

    def _stage(self, ctx, x, policy=SCHEDULED):
        """Hand the batch (from _prep_input) to the context: returns (xp, read), xp the device
        pointer the entry point takes -- None for a batch staged in the context ("the staged batch",
        include/explainn_hip.h) -- and read True when nothing is left for _settle: the validation
        flag was read here, or the batch takes the dense kernels, which flag nothing.
        Base codes are always staged.  An fp32 batch follows `policy`:
          SCHEDULED       when this call validates (validate_input), staged and its flag read BEFORE
                          anything is computed from it: a batch that is not one-hot (the reference
                          accepts any float tensor, architectures/__init__.py:111) goes through the
                          dense kernels instead of being run as if its soft columns were N -- unless
                          dense_input is False, which keeps the strict error.  Otherwise the batch is
                          packed inside the launch itself and the flag stays sticky on the device for
                          a later read (no host sync in the call);
          VALIDATE_FIRST  always validated as above;
          ONEHOT_ONLY     staged and validated; dense_input or a batch that is not one-hot raises."""
        lib, h = ctx.lib, ctx.handle
        if isinstance(x, _SequenceRows):
            # base codes that the entry point stages itself, sub-batch by sub-batch: the flag stays
            # sticky for _settle, as for BaseCodes
            self._rt.calls += 1
            _lib.check(lib.explainn_dense_input(h, 0))
            return x.codes.data_ptr(), False
        if isinstance(x, BaseCodes):
            self._rt.calls += 1
            _lib.check(lib.explainn_dense_input(h, 0))
            ctx.call("explainn_stage_codes", x.codes, x.codes.shape[0], int(x.reverse_complement))
            return None, False
        if self.dense_input:
            if policy == ONEHOT_ONLY:
                raise ValueError("in_silico_mutagenesis and integrated_gradients need one-hot input "
                                 "(dense_input is True)")
            self._rt.calls += 1
            _lib.check(lib.explainn_dense_input(h, 1))
            self._rt.x_keep = x
            return x.data_ptr(), True
        self._rt.calls += 1
        if policy == SCHEDULED and not self._validate_now():
            _lib.check(lib.explainn_dense_input(h, 0))
            return x.data_ptr(), False
        ctx.call("explainn_stage_onehot", x, x.shape[0])
        flags = C.c_int(0)
        ctx.call("explainn_input_flags", C.byref(flags))
        if flags.value & 1:
            if policy == ONEHOT_ONLY:
                raise ValueError(
                    "input is not one-hot: in-silico mutagenesis substitutes bases of one-hot (A,C,G,T) "
                    "or all-zero (N) columns, as sequence.one_hot_encode produces (integrated_gradients "
                    "walks its path between such columns too)")
            self._rt.soft_seen = True
            if self.dense_input is False:
                raise ValueError(
                    "input is not one-hot: every column of x must be one-hot (A,C,G,T) or all-zero "
                    "(N) as sequence.one_hot_encode produces (dense_input=False forbids the dense path)")
            _lib.check(lib.explainn_dense_input(h, 1))
            self._rt.x_keep = x                # the backward of a train forward reads x again
            return x.data_ptr(), True
        _lib.check(lib.explainn_dense_input(h, 0))
        return None, True

    def _front(self, x, dev, policy=SCHEDULED, bump=True):
        """Front half of a launch, inside the caller's torch.cuda.device(dev) with x from
        _prep_input: bump the token (an eval launch overwrites the scratch of a train forward still
        awaiting its backward; train forwards bump it after their launch instead), resolve context
        and params table, and stage x.  Returns (ctx, ps, keep, xp, read); the entry point makes
        its call and hands `read` to _settle -- _launch is the two halves around a body."""
        if bump:
            self._rt.token += 1
        ctx = self._context(x.shape[0], dev)
        ps, keep = self._params_struct(dev)
        xp, read = self._stage(ctx, x, policy)
        return ctx, ps, keep, xp, read

    @contextlib.contextmanager
    def _launch(self, x, dev, policy=SCHEDULED, bump=True):
        """The scope of one launch: torch.cuda.device(dev), _front, the body with (ctx, ps, xp) -- its
        calls go through ctx.call -- then _settle.  A body that raises is not settled."""
        with torch.cuda.device(dev):
            ctx, ps, _, xp, read = self._front(x, dev, policy, bump)
            yield ctx, ps, xp
            self._settle(read)

    def _settle(self, read):
        """Back half of a launch: read the sticky flag when _stage has not and the schedule says
        this call reads it (base codes and deferred fp32 batches; every VALIDATE_EVERY-th call
        settles the deferred ones)."""
        if not read and self.validate_input and (
                self._validate_now() or self._rt.calls % VALIDATE_EVERY == 0):
            self.check_input()

    def _stream(self, dev):
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def check_input(self, also=0):
        """Read (one host sync) and clear the sticky validation flag; raise if any batch since the
        last read was not one-hot.  predict(), Trainer validation passes and the filter export call
        it after their loops.  also: the flags already read of another context (the replica's)."""
        if (self.input_flags() | also) & 1:
            raise ValueError(
                "input is not one-hot: base codes must be 0..4, and every column of an fp32 x must "
                "be one-hot (A,C,G,T) or all-zero (N) as sequence.one_hot_encode produces.  A batch "
                "since the last check was run with such columns read as N; for soft (real-valued) "
                "input set model.dense_input = True, or validate_input = 'always' to route per batch")

    def input_flags(self):
        """Synchronise and return (then clear) the device-side input validation flags."""
        ctx = self._rt.ctx
        if ctx is None:
            return 0
        dev = self._device()
        flags = C.c_int(0)
        with torch.cuda.device(dev):
            ctx.call("explainn_input_flags", C.byref(flags))
        return flags.value

    # -- forward / backward ---------------------------------------------------------------
    def forward(self, x):
        """Forward propagation of a batch: (B,4,L) one-hot -> (B,T) logits."""
        dev = self._device()
        if self.training:
            if torch.is_grad_enabled():
                return _TrainStep.apply(self, x, *self.parameters())
            return self._launch_train(x)[0]
        if torch.is_grad_enabled() and torch.is_tensor(x) and x.requires_grad and x.shape[0] > 0:
            return _EvalInputGrad.apply(self, x)
        x = self._prep_input(x, dev)
        B = x.shape[0]
        logits = self._logits_empty(B, dev)
        if B == 0:                                   # torch returns an empty (0, T) tensor in eval
            return logits
        with self._launch(x, dev) as (ctx, ps, xp):
            ctx.call("explainn_forward_eval", xp, B, ps, logits)
        return logits

    def _launch_scan(self, win, mode=_lib.SCAN_AUTO):
        """Eval-mode logits of the windows of a SequenceWindows (explainn_scan): (n_windows, T) --
        (n_windows, G, T) on a bank -- fp32 on the device, row i the logit of window i (of its reverse
        complement when win.reverse_complement).  The shared track's workspace comes from torch's
        caching allocator."""
        if self.training:
            raise RuntimeError("a scan is an eval-mode path; call model.eval()")
        dev = self._device()
        win.check(dev)
        logits = self._logits_empty(win.n_windows, dev)
        if win.n_windows == 0:
            return logits
        with self._launch(win, dev) as (ctx, ps, xp):
            ws, nbytes = ctx.workspace("explainn_scan_workspace_bytes", win.n_windows, win.stride, mode)
            ctx.call("explainn_scan", xp, win.codes.numel(), win.start, win.n_windows, win.stride,
                     int(win.reverse_complement), ps, logits, mode, ws, nbytes)
        return logits

    def _launch_score_rows(self, rows, symbol, noun, want_outs):
        """Eval-mode logits of the rows of an EditedWindows / HaplotypeWindows through the entry point
        `symbol`: (rows, T) -- (rows, G, T) on a bank -- fp32 on the device; with want_outs also the
        per-unit outputs (rows, units), units = G*U on a bank, from the same pass: returns (logits, outs)."""
        if self.training:
            raise RuntimeError("scoring %s is an eval-mode path; call model.eval()" % noun)
        dev = self._device()
        rows.check(dev)
        logits = self._logits_empty(rows.n_rows, dev)
        outs = torch.empty(rows.n_rows, self._units(), device=dev, dtype=torch.float32) if want_outs else None
        if rows.n_rows > 0:
            with self._launch(rows, dev) as (ctx, ps, xp):
                ctx.call(symbol, xp, rows.codes.numel(), rows.struct(), rows.n_rows, int(rows.reverse_complement),
                         ps, logits, outs)
        return (logits, outs) if want_outs else logits

    def _launch_score_edits(self, ew, want_outs=False):
        """_launch_score_rows of an EditedWindows (explainn_score_edits)."""
        return self._launch_score_rows(ew, "explainn_score_edits", "edits", want_outs)

    def _launch_score_haplotypes(self, hw, want_outs=False):
        """_launch_score_rows of a HaplotypeWindows (explainn_score_haplotypes)."""
        return self._launch_score_rows(hw, "explainn_score_haplotypes", "haplotypes", want_outs)

    def _codes_front(self, codes, path, verb, start=0, reverse_complement=False):
        """Front half of the launches that read a device-resident sequence of base codes with the
        eval-mode tables: the eval-mode check (`path` is the message's subject), the check of `codes`
        (`verb` is what is done on them), then _front.  Returns (ctx, ps, xp, dev); the caller
        checks its other arguments and makes its call inside torch.cuda.device(dev)."""
        if self.training:
            raise NotImplementedError("%s an eval-mode export path; call model.eval()" % path)
        dev = self._device()
        _check_codes(codes, dev, verb + " on")
        with torch.cuda.device(dev):
            ctx, ps, _, xp, _ = self._front(SequenceWindows(codes, start, 1, 1, reverse_complement, 1), dev)
        return ctx, ps, xp, dev

    def _launch_call_sites(self, codes, thresholds, start=0, n_positions=None, period=0,
                           reverse_complement=False, capacity=0, pos=None, score=None):
        """Motif sites of a device-resident 1-D uint8 sequence of base codes (explainn_call_sites):
        every (unit, start position p in [start, start + n_positions)) whose float16 activation
        exceeds thresholds[unit] (fp32 (units,), on the device).  Returns (offsets, pos, score) on the
        device: offsets int64 (units+1), the exclusive scan of the full per-unit counts; pos int32
        (start-relative) and score fp32 hold the first `capacity` records, unit by unit in ascending
        position.  capacity 0 counts only (pos and score are None); pos / score may be given as
        buffers of at least `capacity` elements.  n_positions None: every start the sequence holds."""
        ctx, ps, xp, dev = self._codes_front(codes, "calling sites is", "sites are called", start, reverse_complement)
        k, U = self._options["kernel_size"], self._units()
        _lib.require(thresholds, torch.float32, (U,), dev, "thresholds")
        if n_positions is None:
            n_positions = max(codes.numel() - int(start) - k + 1, 0)
        capacity = int(capacity)
        offsets = torch.empty(U + 1, device=dev, dtype=torch.int64)
        if capacity > 0:
            if pos is None:
                pos = torch.empty(capacity, device=dev, dtype=torch.int32)
            if score is None:
                score = torch.empty(capacity, device=dev, dtype=torch.float32)
            for name, t, dt in (("pos", pos, torch.int32), ("score", score, torch.float32)):
                if _lib.require(t, dt, (None,), dev, name).numel() < capacity:
                    raise RuntimeError("%s must hold at least %d elements (holds %d)" % (name, capacity, t.numel()))
        else:
            pos = score = None
        with torch.cuda.device(dev):
            ws, nbytes = ctx.workspace("explainn_call_sites_workspace_bytes", int(n_positions))
            ctx.call("explainn_call_sites", xp, codes.numel(), int(start), int(n_positions), int(period),
                     int(bool(reverse_complement)), ps, thresholds, offsets, pos, score, capacity, ws, nbytes)
        return offsets, pos, score

    def _launch_record_best(self, codes, rec_offsets, strands=2, want_site=True):
        """The best site of every unit in every record (explainn_record_best).  codes: a device-resident
        1-D uint8 tensor of base codes; rec_offsets: int64 (n_records + 1,) on the device, record r being
        codes[rec_offsets[r] : rec_offsets[r + 1]]; strands 1 (forward) or 2 (both).  Returns (bits, site)
        on the device, unit-major (units, n_records): bits int16, the largest float16 activation's bit
        pattern (below 0x8000) over the record's live starts (0 without one), and site int32, (start << 1) | is_minus of
        the site that holds it (-1 without one; None unless want_site)."""
        ctx, ps, xp, dev = self._codes_front(codes, "the best sites are", "best sites are found")
        U = self._units()
        if _lib.require(rec_offsets, torch.int64, (None,), dev, "rec_offsets").numel() < 1:
            raise RuntimeError("rec_offsets must hold n_records + 1 entries (holds none)")
        if strands not in (1, 2):
            raise ValueError("strands must be 1 (forward) or 2 (both)")
        n = rec_offsets.numel() - 1
        bits = torch.empty((U, n), device=dev, dtype=torch.int16)
        site = torch.empty((U, n), device=dev, dtype=torch.int32) if want_site else None
        with torch.cuda.device(dev):
            ctx.call("explainn_record_best", xp, codes.numel(), rec_offsets, n, int(strands), ps, bits, site)
        return bits, site

    def _launch_activation_histogram(self, codes, hist, start=0, n_positions=None, period=0,
                                     reverse_complement=False):
        """Adds, for every unit and every live start p in [start, start + n_positions) of a
        device-resident 1-D uint8 sequence of base codes, one count to hist[unit][bit pattern of the
        float16 activation] (explainn_activation_histogram).  hist: int64 (units, _lib.ACT_BINS) on the
        device, added into.  Live as in _launch_call_sites: with a period, a start whose k-mer would
        cross a record boundary is not counted.  n_positions None: every start the sequence holds.
        Returns hist."""
        ctx, ps, xp, dev = self._codes_front(codes, "the activation null is", "activations are counted", start,
                                             reverse_complement)
        k, U = self._options["kernel_size"], self._units()
        _lib.require(hist, torch.int64, (U, _lib.ACT_BINS), dev, "hist")
        if n_positions is None:
            n_positions = max(codes.numel() - int(start) - k + 1, 0)
        with torch.cuda.device(dev):
            ctx.call("explainn_activation_histogram", xp, codes.numel(), int(start), int(n_positions), int(period),
                     int(bool(reverse_complement)), ps, hist)
        return hist

    def _launch_eval_keep(self, x):
        """Eval forward that keeps what _launch_input_grad needs (explainn_forward_eval_keep: the
        same logits as forward()).  The batch is validated first, so soft input takes the dense
        kernels.  Returns (logits, token)."""
        dev = self._device()
        x = self._prep_input(x, dev)
        B = x.shape[0]
        logits = self._logits_empty(B, dev)
        with self._launch(x, dev, VALIDATE_FIRST) as (ctx, ps, xp):
            self._rt.x_keep = x                # a dense batch is read again by the input gradient
            ctx.call("explainn_forward_eval_keep", xp, B, ps, logits)
        return logits, self._rt.token

    def _launch_input_grad(self, dlogits, token):
        """dx (B,4,L) of the last _launch_eval_keep for d loss / d logits = dlogits."""
        if token != self._rt.token:
            raise RuntimeError("input gradient of a stale forward: the fused kernels keep one forward "
                               "per model (call backward before the next forward)")
        dev = self._device()
        ctx = self._rt.ctx
        ps, keep = self._params_struct(dev)
        dl = dlogits.to(device=dev, dtype=torch.float32).contiguous()
        B = dl.shape[0]
        dx = torch.empty(B, 4, self._options["sequence_length"], device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            ctx.call("explainn_input_grad", dl, B, ps, dx)
        return dx

    def input_gradient(self, x, dlogits):
        """d(sum(dlogits * model(x))) / dx in eval mode, (B,4,L) fp32, without autograd: one
        eval forward and the input-gradient launches.  x as forward() takes it (fp32 one-hot or
        soft, or base codes -- then the gradient is with respect to the one-hot the model ran on,
        the reverse complement's for BaseCodes(..., reverse_complement=True))."""
        if self.training:
            raise RuntimeError("input_gradient is an eval-mode path; call model.eval()")
        _, token = self._launch_eval_keep(x)
        return self._launch_input_grad(dlogits, token)

    def in_silico_mutagenesis(self, x):
        """In-silico mutagenesis in eval mode (explainn_ism): returns (logits (B,T), delta (B,T,4,L)),
        device fp32 tensors, with delta[b,t,a,p] = logit_t(x_b with base a at p) - logit_t(x_b) for
        a = A,C,G,T -- exactly 0 at the reference base -- and logits those of forward(), bit for bit.
        x: fp32 one-hot (B,4,L), validated before anything is computed (a batch that is not one-hot
        raises ValueError: substitutions are defined on one-hot sequences), or base codes; for
        BaseCodes(..., reverse_complement=True) rows and positions are those of the strand the model
        ran on.  The workspace comes from torch's caching allocator."""
        if self.training:
            raise RuntimeError("in_silico_mutagenesis is an eval-mode path; call model.eval()")
        dev = self._device()
        x = self._prep_input(x, dev)
        B = x.shape[0]
        T, L = self._options["n_features"], self._options["sequence_length"]
        logits = torch.empty(B, T, device=dev, dtype=torch.float32)
        delta = torch.empty(B, T, 4, L, device=dev, dtype=torch.float32)
        if B == 0:
            return logits, delta
        with self._launch(x, dev, ONEHOT_ONLY) as (ctx, ps, xp):
            ws, nbytes = ctx.workspace("explainn_ism_workspace_bytes", B)
            ctx.call("explainn_ism", xp, B, ps, logits, delta, ws, nbytes)
        return logits, delta

    def evolve(self, codes, weights, rounds=10, mutable=None, both_strands=False, lock=True, min_gain=0.0):
        """Greedy in-silico evolution in eval mode: `rounds` times, apply to every sequence the single
        substitution that raises sum_t weights[b,t] * logit_t the most -- the mean of the two strands'
        logits with both_strands.  A round is in_silico_mutagenesis() per strand and one selection
        launch (explainn_evolve_pick) that reduces the maps, picks the winner and edits the codes on the
        device.  Maps, codes, mask and log stay there; the rounds are a Python loop, so every
        in_silico_mutagenesis call allocates its workspace and map and validates its input as usual
        (validate_input: a read of the sticky flag, a host sync, on the first calls and every
        VALIDATE_EVERY-th).  codes: a contiguous uint8 (B,L) tensor
        of base codes on the model's device, EDITED IN PLACE.  weights: fp32 (T,) or (B,T).  mutable:
        None or a (B,L) mask, 0 = the position stays as it is.  lock: a substituted position is not
        revisited.  min_gain >= 0: a round moves a sequence only for a gain above it.  Ties go to the
        lowest position, then the lowest base.  Returns (pos int32, ref uint8, alt uint8, gain float64,
        each (rounds, B), and logits (rounds+1, S, B, T) fp32, S = 2 (forward, reverse) with
        both_strands): pos -1 and ref = alt = 255 where a round found no move; logits[r, s] is
        forward() on the codes before round r (logits[rounds]: the result), bit for bit."""
        if self.training:
            raise RuntimeError("evolve is an eval-mode path; call model.eval()")
        rounds = int(rounds)
        if rounds < 1:
            raise ValueError("evolve needs rounds >= 1 (got %d)" % rounds)
        min_gain = float(min_gain)
        if not (min_gain >= 0.0 and min_gain != float("inf")):
            raise ValueError("min_gain must be finite and not negative (got %r)" % min_gain)
        if self.dense_input:
            raise ValueError("evolve substitutes base codes (dense_input is True)")
        dev = self._device()
        T, L = self._options["n_features"], self._options["sequence_length"]
        if not torch.is_tensor(codes) or codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] != L \
                or not codes.is_contiguous():
            raise ValueError("codes must be a contiguous uint8 tensor of shape (B, %d)" % L)
        if codes.device != dev:
            raise RuntimeError("input is on %s but the model is on %s" % (codes.device, dev))
        B, S = codes.shape[0], 2 if both_strands else 1
        w = torch.as_tensor(weights).to(device=dev, dtype=torch.float32).contiguous()
        if tuple(w.shape) not in ((T,), (B, T)):
            raise ValueError("weights must have shape (%d,) or (%d, %d), got %s" % (T, B, T, tuple(w.shape)))
        mask = None
        if mutable is not None:
            if not torch.is_tensor(mutable) or tuple(mutable.shape) != (B, L):
                raise ValueError("mutable must be a tensor of shape (%d, %d)" % (B, L))
            mask = (mutable.to(dev) != 0).to(torch.uint8).contiguous()       # the working copy locking closes
        elif lock:
            mask = torch.ones(B, L, device=dev, dtype=torch.uint8)
        pos = torch.empty(rounds, B, device=dev, dtype=torch.int32)
        ref = torch.empty(rounds, B, device=dev, dtype=torch.uint8)
        alt = torch.empty(rounds, B, device=dev, dtype=torch.uint8)
        gain = torch.empty(rounds, B, device=dev, dtype=torch.float64)
        logits = torch.empty(rounds + 1, S, B, T, device=dev, dtype=torch.float32)
        if B == 0:
            return pos, ref, alt, gain, logits
        with torch.no_grad():
            for r in range(rounds):
                maps = []
                for s in range(S):
                    logits[r, s], delta = self.in_silico_mutagenesis(BaseCodes(codes, bool(s)))
                    maps.append(delta)
                _lib.call("explainn_evolve_pick", dev, maps[0], maps[1] if S == 2 else None, codes, mask, w,
                          int(w.dim() == 2), B, T, L, int(bool(lock)), min_gain, pos[r], ref[r], alt[r], gain[r])
            for s in range(S):
                logits[rounds, s] = self.forward(BaseCodes(codes, bool(s)))
        return pos, ref, alt, gain, logits

    def integrated_gradients_workspace_bytes(self, B):
        """Bytes of workspace integrated_gradients() runs a batch of B sequences with
        (explainn_integrated_gradients_workspace_bytes); the value for B = 64 is the smallest
        workspace the call accepts."""
        dev = self._device()
        with torch.cuda.device(dev):
            ctx = self._context(B, dev)
            return int(ctx.lib.explainn_integrated_gradients_workspace_bytes(ctx.handle, B))

    def integrated_gradients(self, x, dlogits, baseline="zero", steps=32, workspace=None):
        """Integrated Gradients in eval mode (explainn_integrated_gradients): returns (ig (B,4,L),
        logits_x (B,T), logits_base (B,T)), device fp32 tensors, with
        ig = (x - x') * mean over the nodes a_s = (s + 1/2)/steps of d sum(dlogits * model(x_a)) / dx
        along x_a = x' + a (x - x'), in one device pass: the path is walked in the space of the conv
        sums, which are linear in x.  logits_x / logits_base are the logits at the two ends from the
        same pass, so sum(ig) - (dlogits * (logits_x - logits_base)).sum(1) is the convergence delta.
        x: fp32 one-hot (B,4,L), validated before anything is computed, or base codes; for
        BaseCodes(..., reverse_complement=True) rows and positions are those of the strand the model
        ran on, and the baseline codes are reverse-complemented with the batch.
        baseline: "zero" (all-zero columns), "uniform" (0.25 everywhere) or a uint8 (B,L) tensor of base
        codes on the model's device (0..3, 4 = N); where it equals x the result is exactly 0.
        workspace: an optional uint8 device tensor (at least integrated_gradients_workspace_bytes(64)
        bytes: the batch runs in the sub-batches it holds); by default from torch's caching allocator."""
        if self.training:
            raise RuntimeError("integrated_gradients is an eval-mode path; call model.eval()")
        steps = int(steps)
        if steps < 1:
            raise ValueError("integrated_gradients needs steps >= 1 (got %d)" % steps)
        dev = self._device()
        x = self._prep_input(x, dev)
        B = x.shape[0]
        T, L = self._options["n_features"], self._options["sequence_length"]
        codes = None
        if isinstance(baseline, str):
            kinds = {"zero": _lib.IG_BASELINE_ZERO, "uniform": _lib.IG_BASELINE_UNIFORM}
            if baseline not in kinds:
                raise ValueError("baseline must be 'zero', 'uniform' or a uint8 (B, %d) tensor of base codes" % L)
            kind = kinds[baseline]
        else:
            kind = _lib.IG_BASELINE_CODES
            if not torch.is_tensor(baseline) or baseline.dtype != torch.uint8 or tuple(baseline.shape) != (B, L):
                raise ValueError("baseline codes must be a uint8 tensor of shape (%d, %d), got %s" % (
                    B, L, tuple(baseline.shape) if hasattr(baseline, "shape") else type(baseline).__name__))
            if baseline.device != dev:
                raise RuntimeError("baseline is on %s but the model is on %s" % (baseline.device, dev))
            codes = baseline.detach().contiguous()
        dl = dlogits.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(dl.shape) != (B, T):
            raise ValueError("dlogits must have shape (%d, %d), got %s" % (B, T, tuple(dl.shape)))
        ig = torch.empty(B, 4, L, device=dev, dtype=torch.float32)
        lx = torch.empty(B, T, device=dev, dtype=torch.float32)
        lb = torch.empty(B, T, device=dev, dtype=torch.float32)
        if B == 0:
            return ig, lx, lb
        with self._launch(x, dev, ONEHOT_ONLY) as (ctx, ps, xp):
            if workspace is None:
                workspace = ctx.workspace("explainn_integrated_gradients_workspace_bytes", B)[0]
            _lib.require(workspace, torch.uint8, (None,), dev, "workspace")
            ctx.call("explainn_integrated_gradients", xp, B, ps, kind, codes, dl, steps, ig, lx, lb, workspace,
                     workspace.numel())
        return ig, lx, lb

    def _empty_batch_error(self):
        # what torch's BatchNorm1d raises for an empty batch in train mode
        return ValueError("Expected more than 1 value per channel when training, got input size "
                          "[0, %d, 1]" % (FC_HIDDEN * self._units()))

    def _dropout_args(self, dev, B, rank=None):
        """(keep_mask, seed) of a train forward: the mask of set_dropout_mask (consumed here) as the
        kernels take it, or None; a fresh seed for the built-in generator (rank_seed'ed per rank
        under sync-BN), 0 when dropout is off."""
        mask, self._rt.pending = self._rt.pending, None
        if mask is not None:
            mask = mask.to(device=dev, dtype=torch.uint8).contiguous()
            if mask.numel() != B * FC_HIDDEN * self._units():
                raise RuntimeError("keep-mask must have shape (B, 100*cnn_units)")
        if self.dropout_p > 0:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            return mask, seed if rank is None else rank_seed(seed, rank)
        return mask, 0

    def _launch_train_sync(self, x):
        """Sync-BN forward of the autograd path (parallel.sync_batchnorm): phases 1-4 of
        explainn_sync_phase with the reducer's exchanges between them; the backward runs 5-8."""
        red = self.sync_bn
        dev = self._device()
        if self.dense_input:
            raise ValueError("sync-BN works on one-hot input or base codes, not dense_input")
        x = self._prep_input(x, dev)
        B = x.shape[0]
        if B == 0:
            raise self._empty_batch_error()
        Bg = int(red.global_batch(B))
        logits = self._logits_empty(B, dev)
        mask, seed = self._dropout_args(dev, B, red.rank)
        gs = _lib.Grads()
        with torch.cuda.device(dev):
            ctx, ps, keep, xp, read = self._front(x, dev, bump=False)
            bufs = self._rt.sync_bufs = sync_buffers(ctx, dev, self._rt.sync_bufs)
            a = _lib.SyncArgs(x=xp, B_local=B, B_global=Bg, params=C.pointer(ps),
                              grads=C.pointer(gs), dropout_p=float(self.dropout_p), seed=seed,
                              keep_mask=mask.data_ptr() if mask is not None else None,
                              logits=logits.data_ptr())
            for xb in sync_run(ctx, a, bufs, range(1, 5)):
                red.reduce(xb)
            self._settle(read)
        self._touched()
        self._rt.token += 1
        # the struct and everything it points at stay alive until the backward
        self._rt.sync = (a, ps, keep, gs, mask, logits, x, self._rt.token)
        return logits, self._rt.token

    def _launch_backward_sync(self, dlogits, token):
        """Phases 5-8: the user's criterion is a mean over this rank's B_local rows, so its dlogits
        are scaled by B_local/B_global -- the gradient of the global mean, exact for mean-reduction
        losses with any shard sizes.  The 14 gradients come out global: grad_sync does not run."""
        st = self._rt.sync
        if st is None or st[-1] != token:
            raise RuntimeError("sync-BN backward without its sync-BN forward")
        a, ps, keep, _, mask, logits, x, _ = st
        dev = self._device()
        ctx = self._rt.ctx
        _, views, gs = flat_grads(list(self.parameters()), dev)
        dl = dlogits.to(torch.float32).contiguous()
        a.dlogits = dl.data_ptr()
        a.dl_scale = float(a.B_local) / float(a.B_global)
        a.grads = C.pointer(gs)
        a.freeze_top_n_filters = int(self.freeze_top_n_filters)
        with torch.cuda.device(dev):
            for xb in sync_run(ctx, a, self._rt.sync_bufs, range(5, 9)):
                self.sync_bn.reduce(xb)
        self._rt.sync = None
        return views

    def _launch_train(self, x, policy=SCHEDULED):
        if self.sync_bn is not None:
            if torch.is_tensor(x) and x.requires_grad:
                raise NotImplementedError("x.grad is not available with sync-BN (parallel.sync_batchnorm)")
            return self._launch_train_sync(x)
        self._rt.sync = None
        dev = self._device()
        x = self._prep_input(x, dev)
        B = x.shape[0]
        if B == 0:
            raise self._empty_batch_error()
        logits = self._logits_empty(B, dev)
        mask, seed = self._dropout_args(dev, B)
        with self._launch(x, dev, policy, bump=False) as (ctx, ps, xp):
            ctx.call("explainn_forward_train", xp, B, ps, mask, float(self.dropout_p), C.c_uint64(seed), logits)
        self._touched()
        self._rt.token += 1
        return logits, self._rt.token

    def set_dropout_mask(self, keep_mask):
        """Use `keep_mask` ((B,100U), nonzero = keep) instead of the generator for the NEXT
        train-mode forward (parity testing against a recorded reference mask)."""
        self._rt.pending = keep_mask

    def _launch_backward(self, dlogits, token, want_dx=False):
        if token != self._rt.token:
            raise RuntimeError("backward of a stale forward: the fused kernels keep one training "
                               "step in flight per model (call backward before the next forward)")
        if self._rt.sync is not None:
            if want_dx:
                raise NotImplementedError("x.grad is not available with sync-BN (parallel.sync_batchnorm)")
            return self._launch_backward_sync(dlogits, token)
        dev = self._device()
        ctx = self._rt.ctx
        ps, keep = self._params_struct(dev)
        flat, views, gs = flat_grads(list(self.parameters()), dev)
        dl = dlogits.to(torch.float32).contiguous()
        B = dl.shape[0]
        dx = None
        with torch.cuda.device(dev):
            if want_dx:
                dx = torch.empty(B, 4, self._options["sequence_length"], device=dev, dtype=torch.float32)
                ctx.call("explainn_backward_input", dl, B, ps, gs, int(self.freeze_top_n_filters), dx)
            else:
                ctx.call("explainn_backward", dl, B, ps, gs, int(self.freeze_top_n_filters))
        if self.grad_sync is not None:
            self.grad_sync(flat)
        return (views, dx) if want_dx else views

    # -- the façade test.py / interpret.py use -----------------------------------------------
    def _first_four_rows(self, x_rep):
        U = self._units()
        if isinstance(x_rep, BaseCodes) or (torch.is_tensor(x_rep) and x_rep.dtype == torch.uint8):
            return x_rep
        if x_rep.dim() != 3 or x_rep.shape[1] not in (4, 4 * U):
            raise RuntimeError("expected the repeated input (B, 4*cnn_units, L) or (B, 4, L)")
        return x_rep[:, :4, :]

    def _unit_outputs(self, x_rep):
        """`model.linears(x.repeat(1,U,1))` -> per-unit outputs (B,U) (test.py:151)."""
        if self.training:
            raise NotImplementedError("linears(x) is an eval-mode export path; call model.eval()")
        dev = self._device()
        x = self._prep_input(self._first_four_rows(x_rep), dev)
        B = x.shape[0]
        outs = torch.empty(B, self._units(), device=dev, dtype=torch.float32)
        with self._launch(x, dev) as (ctx, ps, xp):
            ctx.call("explainn_unit_outputs", xp, B, ps, outs)
        return outs

    def _unit_activations(self, x_rep):
        """`model.linears[:3](x.repeat(1,U,1))` -> exp(BN(conv)) (B,U,L-k+1) (test.py:159-160)."""
        if self.training:
            raise NotImplementedError("linears[:3](x) is an eval-mode export path; call model.eval()")
        dev = self._device()
        x = self._prep_input(self._first_four_rows(x_rep), dev)
        B = x.shape[0]
        o = self._options
        acts = torch.empty(B, self._units(), o["sequence_length"] - o["kernel_size"] + 1,
                           device=dev, dtype=torch.float32)
        with self._launch(x, dev) as (ctx, ps, xp):
            ctx.call("explainn_unit_activations", xp, B, ps, acts)
        return acts

    # -- filter -> PWM export (interpret.py:363-459 on the device; see explainn_amd/interpret.py) --
    def _export_args(self, x, select):
        if self.training:
            raise NotImplementedError("the filter export runs in eval mode; call model.eval()")
        dev = self._device()
        x = self._prep_input(x, dev)
        B = x.shape[0]
        if select is not None:
            if select.shape != (B,) or select.device != dev:
                raise RuntimeError("select must be a (B,) tensor on the model's device")
            select = select.to(torch.uint8).contiguous()
        self._rt.token += 1        # (here, not in _front: before filter_sites checks its accumulators)
        return dev, x, B, select

    def filter_act_max(self, x, unit_max, select=None):
        """unit_max[u] (float32 [U], zeroed by the caller before the first batch) <- running max of
        the float16-rounded eval-mode activations of the selected sequences of this batch."""
        dev, x, B, select = self._export_args(x, select)
        _lib.require(unit_max, torch.float32, (self._units(),), dev, "unit_max")
        with self._launch(x, dev, bump=False) as (ctx, ps, xp):
            ctx.call("explainn_filter_act_max", xp, B, ps, select, unit_max)
        return unit_max

    def filter_sites(self, x, thresholds, site_total, pfm, select=None, site_cap=1000000,
                     want_hit=False):
        """Accumulate this batch's sites into pfm (int32 (U,k,4)) / site_total (int32 [U]); returns
        the (B,U) uint8 "has a site" matrix when want_hit."""
        dev, x, B, select = self._export_args(x, select)
        o = self._options
        U, k = self._units(), o["kernel_size"]
        _lib.require(thresholds, torch.float32, (U,), dev, "thresholds")
        _lib.require(site_total, torch.int32, (U,), dev, "site_total")
        _lib.require(pfm, torch.int32, (U, k, 4), dev, "pfm")
        hit = torch.empty(B, U, device=dev, dtype=torch.uint8) if want_hit else None
        with self._launch(x, dev, bump=False) as (ctx, ps, xp):
            ctx.call("explainn_filter_sites", xp, B, ps, select, thresholds, int(site_cap), site_total, pfm, hit)
        return hit


class _BankCombiner(nn.Module):
    """The `final` layers of a bank's members, stacked: weight (G,T,U), bias (G,T)."""

    def __init__(self, n_models, n_features, cnn_units):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(n_models, n_features, cnn_units))
        self.bias = nn.Parameter(torch.zeros(n_models, n_features))

    forward = _GroupedTaps.forward


class ExplaiNNBank(ExplaiNN):
    """A model bank: `n_models` (G) independently initialised ExplaiNN models of `cnn_units` (U) units
    each, trained on the same batches and targets in ONE fused step (explainn_create_bank) -- the N
    runs of train.py's --initialize, an ensemble, a seed study.  Up to the combiner the members are
    one filter bank of G*U independent units; member g owns units [g*U, (g+1)*U).

    Same sub-module names as ExplaiNN with stacked tensors (member-major): every per-unit tensor has
    G*U where a single model has U, `final.weight` is (G,T,U), `final.bias` (G,T); `parameters()` are
    the same 14 tensors in the same order, so FusedAdam, flat_grads and StepEngine work unchanged.
    `num_batches_tracked` is one scalar per BatchNorm (all members step together).  `bank(x)` gives
    (B,G,T) logits in eval and train mode; the targets of a StepEngine step are shared (B,T) and its
    loss has G values.  `freeze_top_n_filters = n` freezes rows [0,n) of every member; the keep-mask of
    set_dropout_mask is (B, 100*G*U).

    Under the same torch seed the bank holds exactly the parameters of
    `[ExplaiNN(...) for _ in range(n_models)]` built in that order.  `member(g)` gives a stand-alone
    ExplaiNN with copies of member g's tensors.  What works on one model only -- x.grad,
    input_gradient, in_silico_mutagenesis, sync-BN -- raises ValueError: run it on member(g)."""

    def __init__(self, n_models, cnn_units, kernel_size, sequence_length, n_features=1):
        if n_models < 1:
            raise ValueError("n_models must be positive")
        # the members first, drawing from the global generator exactly as a sequence of ExplaiNN
        # constructors does; the stacked skeleton then draws from a forked generator
        members = [ExplaiNN(cnn_units, kernel_size, sequence_length, n_features) for _ in range(n_models)]
        with torch.random.fork_rng(devices=[]):
            super().__init__(n_models * cnn_units, kernel_size, sequence_length, n_features)
        self._groups = n_models
        self._options = {"n_models": n_models, "cnn_units": cnn_units, "kernel_size": kernel_size,
                         "sequence_length": sequence_length, "n_features": n_features,
                         "weights_file": None}
        self.final = _BankCombiner(n_models, n_features, cnn_units)
        for g, m in enumerate(members):
            self.load_member(g, m.state_dict())

    @classmethod
    def from_models(cls, models):
        """The bank whose member g holds copies of models[g]'s parameters and buffers (all of one
        shape, on the CPU or not: the bank is built on the CPU); num_batches_tracked from models[0]."""
        models = list(models)
        o = models[0]._options
        geom = (o["cnn_units"], o["kernel_size"], o["sequence_length"], o["n_features"])
        for m in models:
            mo = m._options
            if (mo["cnn_units"], mo["kernel_size"], mo["sequence_length"], mo["n_features"]) != geom:
                raise ValueError("the members of a bank share (cnn_units, kernel_size, sequence_length, n_features)")
        with torch.random.fork_rng(devices=[]):
            bank = cls(len(models), *geom)
        for g, m in enumerate(models):
            bank.load_member(g, m.state_dict())
        with torch.no_grad():
            for key, v in models[0].state_dict().items():
                if key.endswith("num_batches_tracked"):
                    bank.state_dict()[key].copy_(v)
        return bank

    # -- members ---------------------------------------------------------------------------
    def _member_options(self):
        o = self._options
        return {"cnn_units": o["cnn_units"], "kernel_size": o["kernel_size"],
                "sequence_length": o["sequence_length"], "n_features": o["n_features"],
                "weights_file": None}

    def _member_view(self, key, tensor, g):
        """Member g's part of the stacked tensor `tensor` of state_dict key `key` (a view)."""
        if key.endswith("num_batches_tracked"):
            return tensor
        if key.startswith("final."):
            return tensor[g]
        chunk = tensor.shape[0] // self._groups
        return tensor[g * chunk:(g + 1) * chunk]

    def _check_member(self, g):
        if not 0 <= g < self._groups:
            raise IndexError("member %d of a bank of %d" % (g, self._groups))

    def member_state_dict(self, g):
        """Member g's tensors as the reference-compatible state_dict of a stand-alone ExplaiNN (copies)."""
        self._check_member(g)
        return OrderedDict((key, self._member_view(key, v, g).detach().clone())
                           for key, v in self.state_dict().items())

    def load_member(self, g, state_dict):
        """Copy a stand-alone model's state_dict into member g (num_batches_tracked, shared by the
        bank, is left as it is)."""
        self._check_member(g)
        own = self.state_dict()
        missing = [key for key in own if key not in state_dict and not key.endswith("num_batches_tracked")]
        if missing:
            raise KeyError("state_dict lacks %s" % ", ".join(missing))
        with torch.no_grad():
            for key, v in own.items():
                if key.endswith("num_batches_tracked"):
                    continue
                dst = self._member_view(key, v, g)
                dst.copy_(state_dict[key].reshape(dst.shape))
        self.invalidate()

    def member(self, g):
        """A stand-alone ExplaiNN holding copies of member g's parameters and buffers, on the bank's
        device and in its mode, with its dropout / freeze / input settings."""
        o = self._member_options()
        with torch.random.fork_rng(devices=[]):
            m = ExplaiNN(o["cnn_units"], o["kernel_size"], o["sequence_length"], o["n_features"])
        m.load_state_dict(self.member_state_dict(g))
        m.to(self.final.weight.device)
        m.train(self.training)
        m.dropout_p = self.dropout_p
        m.freeze_top_n_filters = self.freeze_top_n_filters
        m.validate_input = self.validate_input
        m.dense_input = self.dense_input
        return m

    # -- what a bank does not do -------------------------------------------------------------
    @staticmethod
    def _member_only(what):
        return ValueError("%s is not available on a model bank: run it on one member, bank.member(g)" % what)

    @property
    def sync_bn(self):
        return None

    @sync_bn.setter
    def sync_bn(self, reducer):
        if reducer is not None:
            raise self._member_only("sync-BN")

    def forward(self, x):
        """(B,4,L) one-hot or base codes -> (B,G,T): member g's logits at [:, g]."""
        if torch.is_tensor(x) and x.requires_grad:
            raise self._member_only("x.grad")
        return super().forward(x)

    def input_gradient(self, x, dlogits):
        raise self._member_only("input_gradient")

    def in_silico_mutagenesis(self, x):
        raise self._member_only("in_silico_mutagenesis")

    def integrated_gradients(self, x, dlogits, baseline="zero", steps=32, workspace=None):
        raise self._member_only("integrated_gradients")

    def evolve(self, codes, weights, rounds=10, mutable=None, both_strands=False, lock=True, min_gain=0.0):
        raise self._member_only("evolve")

    # -- plumbing --------------------------------------------------------------------------
    def _units(self):
        return self._groups * self._options["cnn_units"]

    def _logits_empty(self, B, dev):
        return torch.empty(B, self._groups, self._options["n_features"], device=dev, dtype=torch.float32)


class PWM(nn.Module):
    """Frozen position-weight-matrix scanner, the reference's `PWM` (architectures/__init__.py:
    116-170): `pwms` (G,4,k) in ACGT row order, both strands, per-sequence max or sum of the window
    scores -> (B,G).  `conv1d.weight` / `conv1d.bias` keep the reference's state_dict layout; the
    scan itself is one HIP launch (csrc/pwm.hip), there is no CPU fallback."""

    def __init__(self, pwms, sequence_length, scoring="sum"):
        super().__init__()
        pwms = np.asarray(pwms, dtype=np.float32)
        groups, four, kernel_size = pwms.shape
        if four != 4:
            raise ValueError("pwms must have shape (n, 4, length)")
        self._options = {"groups": groups, "kernel_size": kernel_size,
                         "sequence_length": sequence_length, "scoring": scoring}
        self.conv1d = _GroupedTaps(groups, 4, kernel_size)
        self.conv1d.weight.data = torch.from_numpy(pwms.copy())
        self.conv1d.bias.data = torch.zeros(groups)
        for p in self.conv1d.parameters():
            p.requires_grad = False

    def forward(self, x):
        o = self._options
        w = self.conv1d.weight
        if w.device.type != "cuda":
            raise RuntimeError("explainn_amd.PWM runs only on a HIP device; call .cuda()")
        if x.dim() != 3 or x.shape[1] != 4 or x.shape[2] != o["sequence_length"] or x.device != w.device:
            raise RuntimeError("expected input of shape (B, 4, %d) on %s" % (o["sequence_length"], w.device))
        x = x.detach().to(torch.float32).contiguous()
        scores = torch.empty(x.shape[0], o["groups"], device=w.device, dtype=torch.float32)
        _lib.call("explainn_pwm_scan", w.device, x, x.shape[0], o["sequence_length"], w.detach().contiguous(),
                  o["groups"], o["kernel_size"], _lib.PWM_MAX if o["scoring"] == "max" else _lib.PWM_SUM, scores)
        # the reference adds conv1d.bias (zeros by construction) to every window score
        windows = 1 if o["scoring"] == "max" else 2 * (o["sequence_length"] - o["kernel_size"] + 1)
        return scores.add_(self.conv1d.bias.detach() * windows)


# ----------------------------------------------------------------------------------------------
def get_loss(input_data="binary"):
    """architectures/__init__.py:446-456."""
    if input_data == "binary":
        return nn.BCEWithLogitsLoss()
    return nn.MSELoss()


def get_metrics(input_data="binary"):
    """architectures/__init__.py:458-461."""
    if input_data == "binary":
        from sklearn.metrics import average_precision_score, roc_auc_score
        return dict(aucROC=roc_auc_score, aucPR=average_precision_score)
    from scipy.stats import pearsonr, spearmanr
    return dict(Pearson=pearsonr, Spearman=spearmanr)


def get_optimizer(params, lr=1e-03):
    """architectures/__init__.py:463-464: Adam with torch's defaults.  The object returned is a
    torch.optim.Adam whose step() runs as one HIP launch (optim.FusedAdam)."""
    from .optim import FusedAdam
    return FusedAdam(params, lr=lr)
