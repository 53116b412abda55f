"""Both strands of a sequence, as predict(), scan(), call_sites() and the variant scorers run them:
the forward strand on the model, the reverse complement on its eval_replica() (same tensors, own
device context) on a second stream, so that the launches of one strand fill the gaps between the
dependent launches of the other."""
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


class TwoStrands:
    """with TwoStrands(model, both) as ts: the eval tables of the model (and, with `both`, of its
    replica) are folded once for the block, nothing records gradients, and a clean exit settles input
    validation by ONE read of each context's sticky device flag.  cur is the caller's stream; rep and
    side, the replica and its stream, are None for the forward strand alone."""

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
        self._scopes = [torch.no_grad(), self.model.eval_cache()]
        if self.rep is not None:
            self._scopes.append(self.rep.eval_cache())
        for scope in self._scopes:                      # (none of the three can fail to open)
            scope.__enter__()
        return self

    def __exit__(self, *exc):
        for scope in reversed(self._scopes):
            scope.__exit__(*exc)
        if exc[0] is None and self.model.validate_input:
            # both flags are read (and cleared) before either raises: a raise from the replica's must not
            # leave the model's set for a later call to trip over
            self.model.check_input(self.rep.input_flags() if self.rep is not None else 0)

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
