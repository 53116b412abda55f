"""Greedy in-silico evolution of sequences with a trained ExplaiNN.

    python -m explainn_amd.design MODEL_FILE FASTA [--target T] [--minimize] [--rounds R] [-r]
                                  [--region START:END] [--allow-revisit] [--min-gain G] [-b N]
                                  -o OUT.tsv [--fasta OUT.fa]

Each round applies to every sequence the single-base substitution that moves the chosen logit the most
(ExplaiNN.evolve: the ISM map is reduced and the edit made on the device, round after round).  The
reference has no design command line; this one and its output format are this package's own.
OUT.tsv has one row per accepted substitution,
    SeqId  Round  Pos  Ref  Alt  Gain  Score
Pos 0-based, Gain the predicted change of the objective, Score the objective after the move; rounds
without a move are left out.  --fasta writes the evolved sequences.  -r optimises the mean of the two
strands' logits, predict()'s Mean column before the sigmoid.  --region limits the substitutions to
positions START <= p < END; --allow-revisit lets a later round change a position again.
"""
import argparse

import numpy as np
import torch

from .strands import eval_pass

LETTERS = "ACGTN"


class Evolution:
    """What evolve() returns, numpy on the host: N sequences, R rounds, S strands, T tasks.
      codes   (N,L) uint8      the evolved sequences
      pos     (N,R) int32      position of round r's substitution, -1: no move
      ref     (N,R) uint8      the base it replaced (4 = N), 255: no move
      alt     (N,R) uint8      the base it wrote, 255: no move
      gain    (N,R) float64    the objective's predicted change (from the ISM map), 0: no move
      logits  (N,R+1,S,T) float32  eval-mode logits before round r (index R: of the result); S = 2
                               (forward, reverse complement) with rev_complement
      score   (N,R+1) float64  the objective of those logits: sum_t w_t * (mean over strands)"""

    def __init__(self, codes, pos, ref, alt, gain, logits, weights):
        self.codes, self.pos, self.ref, self.alt, self.gain, self.logits = codes, pos, ref, alt, gain, logits
        self.weights = weights                                    # (T,) or (N,T) float32, sign included
        w = weights.astype(np.float64)
        w = w[None, None, :] if w.ndim == 1 else w[:, None, :]
        self.score = (logits.astype(np.float64).mean(axis=2) * w).sum(axis=2)

    def mutations(self):
        """The accepted substitutions as a flat list of (sequence, round, pos, ref, alt, gain, score
        after the move), by sequence, then round; ref and alt as letters."""
        out = []
        for i, r in zip(*np.nonzero(self.pos >= 0)):
            out.append((int(i), int(r), int(self.pos[i, r]), LETTERS[min(int(self.ref[i, r]), 4)],
                        LETTERS[int(self.alt[i, r])], float(self.gain[i, r]), float(self.score[i, r + 1])))
        return out

    def sequences(self):
        """The evolved sequences as strings."""
        lut = np.frombuffer(LETTERS.encode(), dtype=np.uint8)
        return [lut[np.minimum(row, 4)].tobytes().decode() for row in self.codes]


def _as_codes(codes):
    """(N,L) uint8 base codes as a tensor (host or device), from codes or from an (N,4,L) one-hot whose
    every column is one-hot or all-zero (N)."""
    if torch.is_tensor(codes) and codes.dtype == torch.uint8 and codes.dim() == 2:
        return codes
    arr = codes.detach().cpu().numpy() if torch.is_tensor(codes) else np.asarray(codes)
    if arr.dtype == np.uint8 and arr.ndim == 2:
        return torch.from_numpy(np.ascontiguousarray(arr))
    if arr.ndim != 3 or arr.shape[1] != 4:
        raise ValueError("codes must be (N,L) uint8 base codes or an (N,4,L) one-hot, got %s %s"
                         % (arr.dtype, arr.shape))
    from .interpret import _onehot_to_codes
    out = _onehot_to_codes(arr)
    if ((out == 4) & (arr != 0).any(axis=1)).any():
        raise ValueError("input is not one-hot: evolution substitutes bases of one-hot (A,C,G,T) or all-zero "
                         "(N) columns")
    return torch.from_numpy(out)


def evolve(model, codes, target=None, rounds=10, maximize=True, mutable=None, rev_complement=False,
           lock=True, min_gain=0.0, batch_size=4096):
    """Greedy in-silico evolution in eval mode: an Evolution.

    codes: (N,L) uint8 base codes (0..3 = A,C,G,T, 4 = N; numpy or tensor, host or device) or an (N,4,L)
    one-hot.  target: a task index, a (T,) weight vector or an (N,T) weight matrix; the objective is
    sum_t w_t * logit_t, None meaning the only task of a one-task model.  maximize=False negates the
    weights.  mutable: None, an (L,) or an (N,L) mask, 0 = the position stays as it is.
    rev_complement=True optimises the mean of the two strands' logits.  lock: a substituted position is
    not revisited.  min_gain >= 0: a sequence moves only for a gain above it.  The sequences run in
    batches of batch_size through one context; a batch's maps, codes and log stay on the device over
    its rounds (ExplaiNN.evolve) and only its results come back."""
    if model.training:
        raise RuntimeError("evolve is an eval-mode path; call model.eval()")
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError("evolve needs rounds >= 1 (got %d)" % rounds)
    T, L = model._options["n_features"], model._options["sequence_length"]
    data = _as_codes(codes)
    if data.shape[1] != L:
        raise ValueError("sequences are %d bp, the model takes %d" % (data.shape[1], L))
    N = data.shape[0]
    if target is None:
        if T != 1:
            raise ValueError("the model has %d tasks: give target (a task index or weights)" % T)
        w = np.ones(1, dtype=np.float32)
    elif np.ndim(target) == 0:
        if not 0 <= int(target) < T:
            raise ValueError("target must be a task index in [0, %d)" % T)
        w = np.zeros(T, dtype=np.float32)
        w[int(target)] = 1.0
    else:
        w = np.asarray(target.detach().cpu() if torch.is_tensor(target) else target, dtype=np.float32)
        if w.shape not in ((T,), (N, T)):
            raise ValueError("target weights must have shape (%d,) or (%d, %d), got %s" % (T, N, T, w.shape))
    if not maximize:
        w = -w
    if mutable is not None:
        mutable = np.asarray(mutable.detach().cpu() if torch.is_tensor(mutable) else mutable) != 0
        if mutable.shape not in ((L,), (N, L)):
            raise ValueError("mutable must have shape (%d,) or (%d, %d), got %s" % (L, N, L, mutable.shape))
        mutable = np.ascontiguousarray(np.broadcast_to(mutable, (N, L))).astype(np.uint8)
    dev = model._device()
    S, batch_size = 2 if rev_complement else 1, max(1, int(batch_size))
    res = dict(codes=np.empty((N, L), np.uint8), pos=np.empty((N, rounds), np.int32),
               ref=np.empty((N, rounds), np.uint8), alt=np.empty((N, rounds), np.uint8),
               gain=np.empty((N, rounds), np.float64), logits=np.empty((N, rounds + 1, S, T), np.float32))
    with eval_pass(model):
        for i in range(0, N, batch_size):
            j = min(i + batch_size, N)
            cb = data[i:j].to(dev).clone().contiguous()           # evolve() edits it in place
            wb = torch.from_numpy(w if w.ndim == 1 else np.ascontiguousarray(w[i:j]))
            mb = torch.from_numpy(mutable[i:j]) if mutable is not None else None
            pos, ref, alt, gain, logits = model.evolve(cb, wb, rounds, mb, rev_complement, lock, min_gain)
            res["codes"][i:j] = cb.cpu().numpy()
            for key, t in (("pos", pos), ("ref", ref), ("alt", alt), ("gain", gain)):
                res[key][i:j] = t.cpu().numpy().T
            res["logits"][i:j] = logits.permute(2, 0, 1, 3).cpu().numpy()
    return Evolution(weights=w, **res)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.design", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model_file")
    ap.add_argument("fasta_file")
    ap.add_argument("--target", type=int, default=None, help="task index (default: the only task)")
    ap.add_argument("--minimize", action="store_true")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("-r", "--rev-complement", action="store_true")
    ap.add_argument("--region", default=None, metavar="START:END")
    ap.add_argument("--allow-revisit", action="store_true")
    ap.add_argument("--min-gain", type=float, default=0.0)
    ap.add_argument("-b", "--batch-size", type=int, default=4096)
    ap.add_argument("-o", "--output-file", required=True)
    ap.add_argument("--fasta", default=None, metavar="OUT.fa")
    args = ap.parse_args(argv)
    from .loader import read_fasta_codes
    from .predict import _load_model
    codes, ids = read_fasta_codes(args.fasta_file)
    model = _load_model(args.model_file)
    L = model._options["sequence_length"]
    if codes.shape[1] != L:
        raise SystemExit("sequences are %d bp, the model takes %d" % (codes.shape[1], L))
    mutable = None
    if args.region is not None:
        try:
            start, end = (int(v) for v in args.region.split(":"))
        except ValueError:
            ap.error("--region takes START:END")
        if not 0 <= start < end <= L:
            ap.error("--region must satisfy 0 <= START < END <= %d" % L)
        mutable = np.zeros(L, dtype=np.uint8)
        mutable[start:end] = 1
    try:
        ev = evolve(model, codes, target=args.target, rounds=args.rounds, maximize=not args.minimize,
                    mutable=mutable, rev_complement=args.rev_complement, lock=not args.allow_revisit,
                    min_gain=args.min_gain, batch_size=args.batch_size)
    except ValueError as e:
        ap.error(str(e))
    with open(args.output_file, "wt") as fh:
        fh.write("SeqId\tRound\tPos\tRef\tAlt\tGain\tScore\n")
        for i, r, p, ref, alt, gain, score in ev.mutations():
            fh.write("%s\t%d\t%d\t%s\t%s\t%s\t%s\n" % (ids[i], r, p, ref, alt, repr(gain), repr(score)))
    if args.fasta:
        with open(args.fasta, "wt") as fh:
            for rid, seq in zip(ids, ev.sequences()):
                fh.write(">%s\n%s\n" % (rid, seq))


if __name__ == "__main__":
    main()
