"""Both strands of a sequence, as predict(), scan(), call_sites() and the variant scorers run them:
the forward strand on the model, the reverse complement on its eval_replica() (same tensors, own
device context) on a second stream, so that the launches of one strand fill the gaps between the
dependent launches of the other.  eval_pass and eval_mode are the scope every eval-mode pass over data
opens, whichever strands it runs."""
import contextlib

import numpy as np
import torch


def as_codes_1d(codes):
    """A sequence of base codes, numpy array or tensor, host or device -> a 1-D uint8 tensor."""
    data = codes if torch.is_tensor(codes) else torch.as_tensor(np.ascontiguousarray(codes))
    if data.dtype != torch.uint8 or data.dim() != 1:
        raise ValueError("codes must be a 1-D uint8 array of base codes")
    return data


def check_strands(strands):
    if strands not in ("both", "fwd"):
        raise ValueError("strands must be 'both' or 'fwd' (got %r)" % (strands,))


def stack_strands(fwd, rev, dim=-1):
    """predict()'s columns [Fwd, Rev, Mean, Max] along a new dimension `dim`.  numpy's float32 mean of
    two values is (a + b) / 2 in float32, as here."""
    return torch.stack((fwd, rev, (fwd + rev) / 2, torch.maximum(fwd, rev)), dim=dim)


@contextlib.contextmanager
def eval_mode(model):
    """The model in eval mode for the block, and back in the mode it was in behind it."""
    was = model.training
    model.eval()
    try:
        yield model
    finally:
        model.train(was)


@contextlib.contextmanager
def eval_pass(model, *others, settle=True):
    """One eval-mode pass over data: nothing records gradients and the eval tables of the model (and of
    `others`: its replica) are folded once for the block.  With `settle`, a clean exit settles input
    validation by ONE read of each context's sticky device flag."""
    with contextlib.ExitStack() as scopes:
        scopes.enter_context(torch.no_grad())
        for m in (model,) + others:
            scopes.enter_context(m.eval_cache())
        yield
    if settle and model.validate_input:
        # every flag is read (and cleared) before anything raises: a raise from the replica's must not
        # leave the model's set for a later call to trip over
        also = 0
        for m in others:
            also |= m.input_flags()
        model.check_input(also)


class TwoStrands:
    """with TwoStrands(model, both) as ts: an eval_pass of the model (and, with `both`, of its
    replica).  cur is the caller's stream; rep and side, the replica and its stream, are None for the
    forward strand alone."""

    def __init__(self, model, both=True):
        device = model.final.weight.device
        self.model, self.cur = model, torch.cuda.current_stream(device)
        self.rep = self.side = None
        if both:
            self.rep = model.eval_replica()
            if model._rt.side_stream is None:
                model._rt.side_stream = torch.cuda.Stream(device)
            self.side = model._rt.side_stream

    def __enter__(self):
        self._scope = eval_pass(self.model, *(() if self.rep is None else (self.rep,)))
        self._scope.__enter__()
        return self

    def __exit__(self, *exc):
        return self._scope.__exit__(*exc)

    def run(self, launch, held=()):
        """launch(m, reverse_complement) on the model and, with both strands, on the replica on the side
        stream at the same time: (fwd, rev), rev None for the forward strand alone.  A launch returns a
        tensor or a tuple of tensors; `held` are the tensors of the caller's stream that the replica
        reads and that may be freed before the side stream is done."""
        rev = None
        if self.rep is not None:
            self.side.wait_stream(self.cur)                 # what the launch reads is on the device
            with torch.cuda.stream(self.side):
                rev = launch(self.rep, True)
            for t in held:
                t.record_stream(self.side)
        fwd = launch(self.model, False)
        if self.rep is not None:
            self.cur.wait_stream(self.side)
            for t in (rev if isinstance(rev, tuple) else (rev,)):
                t.record_stream(self.cur)
        return fwd, rev
