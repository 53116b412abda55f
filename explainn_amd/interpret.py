"""Filter -> PWM interpretation on the device.

Mirrors the part of the reference's interpret.py that turns a trained ExplaiNN into one position
frequency matrix per filter (interpret.py:160-235):

    acts, outs, preds = _get_acts_outs_preds(model, loader)         test.py:128-166
    idxs       = _get_well_predicted_sequences(preds, labels, ...)  interpret.py:310-361
    thresholds = _get_act_thresholds(acts, idxs, rc)                interpret.py:363-373
    sites      = _get_sites(...); motif = _sites_to_motif(sites)    interpret.py:375-459
    imps       = _filter_filter_importances(...)                    interpret.py:485-490

The reference materialises `acts` as a dense float16 (N,U,Lo) host array (11 GB for 100 K sequences
at 300 units / 200 bp) and walks it with Python loops that write FASTA files.  Here the activations
are recomputed inside two HIP passes over the packed base codes (csrc/interpret.hip) and only the
(U,) maxima, the (U,k,4) count matrices and a (N,U) "has a site" bit ever leave the kernel; results
are the same numbers (float16 rounding of the activations included).

`_get_acts_outs_preds` and `_get_well_predicted_sequences` keep the reference's names and argument
meaning; `filter_pwms` replaces the thresholds -> sites -> motif chain.
"""
import argparse
import os
import time

import numpy as np
import torch

from .strands import eval_mode, eval_pass

SITE_CAP = 1000000          # interpret.py:423-424: a filter with 1e6 sites is "way too ubiquitous"


def _get_fwd_rev(arr, strand):
    """test.py:198-203."""
    half = len(arr) // 2
    if strand in ("fwd", "+"):
        return arr[:half]
    if strand in ("rev", "-"):
        return arr[half:]
    raise ValueError("strand must be fwd/+ or rev/-")


def _batches(Xs, batch_size):
    for i in range(0, len(Xs), batch_size):
        yield i, Xs[i:i + batch_size]


def _as_tensor(Xs):
    return Xs if torch.is_tensor(Xs) else torch.as_tensor(np.asarray(Xs), dtype=torch.float32)


def _attribution_input(model, Xs, target):
    """What the attribution drivers open with: `target` checked, Xs as a tensor -- uint8 base codes
    (N,L) as they are, anything else as fp32 (N,4,L).  Returns (Xs, codes, T, L, device), codes True
    for base codes."""
    T, L = model._options["n_features"], model._options["sequence_length"]
    if target is not None and not 0 <= int(target) < T:
        raise ValueError("target must be a task index in [0, %d)" % T)
    codes = (torch.is_tensor(Xs) and Xs.dtype == torch.uint8) or \
        (isinstance(Xs, np.ndarray) and Xs.dtype == np.uint8)
    return torch.as_tensor(Xs) if codes else _as_tensor(Xs), codes, T, L, model.final.weight.device


def _target_dlogits(B, T, target, dev):
    """(B,T) d F / d logits of F = logit[target], or of the sum of the logits with target=None."""
    dl = torch.zeros(B, T, device=dev, dtype=torch.float32)
    if target is None:
        dl.fill_(1.0)
    else:
        dl[:, int(target)] = 1.0
    return dl


def _on_strand(xb, codes, rev_complement):
    """(xb, xin): the device batch as given (one-hot: as fp32) and what the model takes for the chosen
    strand -- codes are staged reverse-complemented, a one-hot batch is flipped here."""
    if codes:
        from .architectures import BaseCodes
        return xb, BaseCodes(xb, rev_complement)
    xb = xb.to(torch.float32)
    return xb, xb.flip(1, 2) if rev_complement else xb


def _get_outs_preds(exp_model, Xs, batch_size=100):
    """The (N,U) unit outputs and (N,T) predictions of test.py:128-166, float16 like there.
    Eval-mode outputs do not depend on batch composition, so the device passes take at least 4096
    sequences whatever batch_size says."""
    batch_size = max(int(batch_size), 4096)
    dev = exp_model.final.weight.device
    U, T = exp_model._options["cnn_units"], exp_model._options["n_features"]
    outputs = np.zeros((len(Xs), U), dtype=np.float16)
    predictions = np.zeros((len(Xs), T), dtype=np.float16)
    Xs = _as_tensor(Xs)
    with eval_pass(exp_model, settle=False):
        for i, xb in _batches(Xs, batch_size):
            outs = exp_model.linears(xb.to(dev))
            outputs[i:i + len(xb)] = outs.cpu().numpy()
            predictions[i:i + len(xb)] = exp_model.final(outs).cpu().numpy()
    return outputs, predictions


def _get_acts_outs_preds(exp_model, data_loader):
    """test.py:128-166, kept for callers that want the dense float16 activation array."""
    o = exp_model._options
    N = len(data_loader.dataset)
    Lo = o["sequence_length"] - o["kernel_size"] + 1
    activations = np.zeros((N, o["cnn_units"], Lo), dtype=np.float16)
    outputs = np.zeros((N, o["cnn_units"]), dtype=np.float16)
    predictions = np.zeros((N, o["n_features"]), dtype=np.float16)
    dev = exp_model.final.weight.device
    idx = 0
    with eval_pass(exp_model, settle=False):
        for Xs, _ in data_loader:
            Xs = Xs.to(dev)
            outs = exp_model.linears(Xs)
            outputs[idx:idx + len(Xs)] = outs.cpu().numpy()
            predictions[idx:idx + len(Xs)] = exp_model.final(outs).cpu().numpy()
            activations[idx:idx + len(Xs)] = exp_model.linears[:3](Xs).cpu().numpy()
            idx += len(Xs)
    return activations, outputs, predictions


def _get_well_predicted_sequences(preds, labels, input_data, rev_complement=False):
    """interpret.py:310-361 (host logic on (N,T) arrays).  Binary data: sequences whose thresholded
    prediction equals the label for every task; otherwise the intersection of the top-5 % labels and
    top-5 % predictions."""
    frac = .05
    if rev_complement:
        fwd, rev = _get_fwd_rev(preds, "fwd"), _get_fwd_rev(preds, "rev")
        ys = _get_fwd_rev(labels, "fwd")
        p = np.empty(fwd.shape)
        for t in range(p.shape[1]):
            p[:, t] = np.mean([fwd[:, t], rev[:, t]], axis=0)
            if input_data == "binary":
                p[:, t] = torch.sigmoid(torch.from_numpy(p[:, t])).numpy()
    else:
        p = torch.sigmoid(torch.from_numpy(preds)).numpy() if input_data == "binary" else preds
        ys = labels
    if input_data == "binary":
        agree = ys == (p > .5).astype(int)
        return np.where(agree.all(axis=1))[0]
    top = int(max(ys.shape) * frac)
    return np.intersect1d(np.argsort(-ys.flatten())[:top], np.argsort(-p.flatten())[:top])


def filter_pwms(exp_model, Xs, idxs, rev_complement=False, batch_size=1024, site_cap=SITE_CAP):
    """thresholds -> sites -> count matrices for every filter, on the device.

    Xs: (N,4,L) one-hot, forward strands followed (when rev_complement) by their reverse complements
    in the same order, as train._get_seqs_labels_ids lays them out; idxs: the well-predicted
    sequence indices (into the forward half when rev_complement).

    Returns dict(thresholds float16 [U], pfm int64 (U,k,4) rows A,C,G,T per site column,
    nsites int64 [U], hit bool (N,U))."""
    o = exp_model._options
    U, k = o["cnn_units"], o["kernel_size"]
    dev = exp_model.final.weight.device
    Xs = _as_tensor(Xs)
    N = len(Xs)
    half = N // 2 if rev_complement else N
    sel = np.zeros(N, dtype=np.uint8)
    idxs = np.asarray(idxs, dtype=np.int64)
    sel[idxs] = 1
    if rev_complement:
        sel[idxs + half] = 1
    select = torch.from_numpy(sel).to(dev)
    with eval_mode(exp_model), eval_pass(exp_model):
        unit_max = torch.zeros(U, device=dev, dtype=torch.float32)
        for i, xb in _batches(Xs, batch_size):
            exp_model.filter_act_max(xb.to(dev), unit_max, select[i:i + len(xb)])
        # interpret.py:373: 0.5 * amax of a float16 array stays float16
        thresholds = (0.5 * unit_max.cpu().numpy().astype(np.float16)).astype(np.float16)
        thr_dev = torch.from_numpy(thresholds.astype(np.float32)).to(dev)
        site_total = torch.zeros(U, device=dev, dtype=torch.int32)
        pfm = torch.zeros(U, k, 4, device=dev, dtype=torch.int32)
        hit = np.zeros((N, U), dtype=bool)
        # forward strand first, then the reverse strand (interpret.py:385-429); a batch never
        # straddles the two halves, so site ranks follow the reference's order
        bounds = [(0, half)] + ([(half, N)] if rev_complement else [])
        for lo, hi in bounds:
            for i in range(lo, hi, batch_size):
                j = min(i + batch_size, hi)
                h = exp_model.filter_sites(Xs[i:j].to(dev), thr_dev, site_total, pfm, select[i:j],
                                           site_cap=site_cap, want_hit=True)
                hit[i:j] = h.cpu().numpy().astype(bool)
    return {"thresholds": thresholds, "pfm": pfm.cpu().numpy().astype(np.int64),
            "nsites": site_total.cpu().numpy().astype(np.int64), "hit": hit}


def _onehot_to_codes(x):
    """(M,4,L) one-hot -> (M,L) uint8 base codes; a column that is not one-hot (all-zero = N) -> 4."""
    x = np.asarray(x)
    onehot = (x.max(axis=1) == 1) & (x.sum(axis=1) == 1)
    return np.where(onehot, x.argmax(axis=1), 4).astype(np.uint8)


def filter_site_list(exp_model, Xs, idxs, thresholds, rev_complement=False, site_cap=SITE_CAP):
    """The site lists behind filter_pwms' count matrices (interpret.py:375-429): for every unit the
    first site_cap sites as an int64 (n,3) array of (sequence index, position, strand).

    Xs, idxs, rev_complement as in filter_pwms; thresholds: (U,), e.g. filter_pwms(...)["thresholds"].
    The selected rows are gathered in idxs order -- with rev_complement the rows of the reverse half
    (idxs + N/2) follow those of the forward half, as the reference iterates -- and flattened to one
    code sequence on which sites.call_sites runs with period = L: a site never crosses two rows.
    Sequence index is the value from idxs; strand is +1 for a forward-half row and -1 for a
    reverse-half row, whose position counts along that (already reverse-complemented) row."""
    from .sites import call_sites
    L = exp_model._options["sequence_length"]
    idxs = np.asarray(idxs, dtype=np.int64)
    half = len(Xs) // 2 if rev_complement else len(Xs)
    rows = np.concatenate([idxs, idxs + half]) if rev_complement else idxs
    U = exp_model._units()
    if len(rows) == 0:
        return [np.zeros((0, 3), dtype=np.int64) for _ in range(U)]
    X = Xs.cpu().numpy() if torch.is_tensor(Xs) else np.asarray(Xs)
    codes = _onehot_to_codes(X[rows]).reshape(-1)
    with eval_mode(exp_model):
        calls = call_sites(exp_model, codes, np.asarray(thresholds, dtype=np.float32), strands="fwd", period=L)
    out = []
    for u in range(U):
        start = calls.unit(u)[0][:site_cap]
        row = start // L
        out.append(np.stack([idxs[row % len(idxs)], start % L,
                             np.where(row < len(idxs), 1, -1)], axis=1).astype(np.int64))
    return out


def site_kmers(Xs, site_list_u, k, rev_complement=False):
    """The k-mer under every site of one unit's list (filter_site_list), read from the row the site was
    found on (the reverse-half row for strand -1); a column that is not one-hot prints as N."""
    half = len(Xs) // 2 if rev_complement else len(Xs)
    X = Xs.cpu().numpy() if torch.is_tensor(Xs) else np.asarray(Xs)
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)
    out = []
    for idx, p, strand in site_list_u:
        row = idx + (half if strand < 0 else 0)
        out.append(letters[_onehot_to_codes(X[row:row + 1, :, p:p + k])[0]].tobytes().decode())
    return out


def write_sites(output_dir, site_lists, kmers, thresholds):
    """The --sites outputs: thresholds.tsv (`filter`, `threshold`: the input of `python -m
    explainn_amd.sites`) and sites/filter<u>.fa, one k-mer per site in list order
    (interpret.py:375-429).  biopython is not available in this image, so the record header
    ('><sequence index>_<strand>_<position>') is a plain restatement and is not pinned by a fixture."""
    from .sites import write_thresholds
    os.makedirs(os.path.join(output_dir, "sites"), exist_ok=True)
    write_thresholds(os.path.join(output_dir, "thresholds.tsv"), thresholds)
    for u, (lst, kms) in enumerate(zip(site_lists, kmers)):
        with open(os.path.join(output_dir, "sites", "filter%d.fa" % u), "wt") as fh:
            for (idx, p, strand), kmer in zip(lst, kms):
                fh.write(">%d_%s_%d\n%s\n" % (idx, "+" if strand > 0 else "-", p, kmer))


def input_gradients(model, Xs, target=None, batch_size=4096, rev_complement=False, times_input=False):
    """Eval-mode input gradients (N,4,L), float32 numpy: d logit[target] / d x -- or d sum(logits)
    / d x with target=None -- for every sequence, what `x.requires_grad_(); model(x)[:, t].sum()
    .backward()` leaves in x.grad on the reference module, in batches on the device with no
    autograd bookkeeping.  The saliency map; times_input=True gives gradient x input.  Integrated
    Gradients are integrated_gradients() below: one device pass along the path, not a loop over this.

    Xs: (N,4,L) one-hot or real-valued (numpy or tensor), or (N,L) uint8 base codes (0..3 = A,C,G,T,
    4 = N).  rev_complement=True runs the model on each sequence's reverse complement and maps the
    gradient back onto the given strand (base and position flipped), so that it multiplies the
    given one-hot."""
    Xs, codes, T, L, dev = _attribution_input(model, Xs, target)
    out = np.zeros((len(Xs), 4, L), dtype=np.float32)
    with eval_mode(model), eval_pass(model):
        for i, xb in _batches(Xs, batch_size):
            xb = xb.to(dev, non_blocking=True)
            B = xb.shape[0]
            dl = _target_dlogits(B, T, target, dev)
            xb, xin = _on_strand(xb, codes, rev_complement)
            dx = model.input_gradient(xin, dl)
            if rev_complement:
                dx = dx.flip(1, 2)
            if times_input and codes:
                onehot = torch.zeros(B, 5, L, device=dev, dtype=torch.float32)
                onehot.scatter_(1, xb.long().clamp(max=4).unsqueeze(1), 1.0)
                dx = dx * onehot[:, :4]
            elif times_input:
                dx = dx * xb
            out[i:i + B] = dx.cpu().numpy()
    return out


def integrated_gradients(model, Xs, baselines="zero", target=None, steps=32, batch_size=4096,
                         rev_complement=False, return_delta=False, n_shuffles=10, seed=0):
    """Integrated Gradients in eval mode, float32 numpy (N,4,L): (x - x') times the mean over `steps`
    midpoint nodes of d logit[target] / dx -- d sum(logits) / dx with target=None -- along the
    straight path from the baseline x' to x, one device pass per batch
    (ExplaiNN.integrated_gradients).

    Xs: (N,4,L) one-hot (numpy or tensor) or (N,L) uint8 base codes (0..3 = A,C,G,T, 4 = N).
    baselines: "zero" (all-zero columns), "uniform" (0.25 in every row: all four rows of a position
    are then generally non-zero), or uint8 base codes (N,L) -- or (N,R,L): R baselines per sequence,
    e.g. sequence.dinucleotide_shuffle(codes, n=R); the result is the mean of the R attributions, each
    multiplied by its own (x - x'_r), accumulated on the device.  "shuffle": n_shuffles
    dinucleotide-preserving shuffles of every sequence, drawn on the device batch by batch
    (sequence.dinucleotide_shuffle_device with `seed` and the batch offset as row0, so the result does
    not depend on batch_size): the same arrays as passing dinucleotide_shuffle_device(codes, n_shuffles,
    seed) as baselines, with nothing but the result crossing to the host.  Its random stream is not the
    host dinucleotide_shuffle's.  One-hot Xs are converted to codes once (a column that is not one-hot
    shuffles as N).  n_shuffles and seed are ignored for every other kind of baseline.
    rev_complement=True runs the model on each sequence's (and baseline's) reverse complement and
    maps base and position back onto the given strand.
    return_delta=True returns (ig, delta), delta (N,) the convergence delta sum(ig) - (F(x) - F(x'))
    (the mean over the R baselines), F the target logit or the sum of the logits."""
    Xs, codes, T, L, dev = _attribution_input(model, Xs, target)
    N = len(Xs)
    base = None
    if not isinstance(baselines, str):
        base = torch.as_tensor(baselines)
        if base.dtype != torch.uint8 or base.dim() not in (2, 3) or base.shape[0] != N or base.shape[-1] != L:
            raise ValueError("baselines must be 'zero', 'uniform' or uint8 base codes of shape (%d, %d) or "
                             "(%d, R, %d), got %s %s" % (N, L, N, L, base.dtype, tuple(base.shape)))
        if base.dim() == 2:
            base = base[:, None]
        if base.shape[1] < 1:
            raise ValueError("baselines holds no baseline per sequence")
    elif baselines not in ("zero", "uniform", "shuffle"):
        raise ValueError("baselines must be 'zero', 'uniform', 'shuffle' or uint8 base codes")
    shuffle = isinstance(baselines, str) and baselines == "shuffle"
    if shuffle:
        if n_shuffles < 1:
            raise ValueError("n_shuffles must be at least 1")
        from .sequence import dinucleotide_shuffle_device
        # the codes the shuffles are drawn from: Xs itself, or the one-hot converted once
        src = Xs if codes else torch.from_numpy(_onehot_to_codes(Xs.cpu().numpy()))
    R = n_shuffles if shuffle else 1 if base is None else base.shape[1]
    out = np.zeros((N, 4, L), dtype=np.float32)
    delta = np.zeros(N, dtype=np.float32)
    with eval_mode(model), eval_pass(model):
        for i, xb in _batches(Xs, batch_size):
            xb = xb.to(dev, non_blocking=True)
            B = xb.shape[0]
            dl = _target_dlogits(B, T, target, dev)
            xb, xin = _on_strand(xb, codes, rev_complement)
            if shuffle:
                cb = xb if codes else src[i:i + B].to(dev, non_blocking=True)
                shuf = dinucleotide_shuffle_device(cb, n_shuffles, seed, row0=i)
            acc = dcc = None
            for r in range(R):
                bl = baselines
                if shuffle or base is not None:
                    bl = shuf[:, r].contiguous() if shuffle else \
                        base[i:i + B, r].to(dev, non_blocking=True).contiguous()
                    if rev_complement and not codes:     # the one-hot batch was flipped here, not staged flipped
                        bl = torch.where(bl < 4, 3 - bl, bl).flip(1)
                ig, lx, lb = model.integrated_gradients(xin, dl, bl, steps)
                d = ig.sum(dim=(1, 2)) - (dl * (lx - lb)).sum(dim=1)
                acc = ig if acc is None else acc.add_(ig)
                dcc = d if dcc is None else dcc.add_(d)
            if R > 1:
                acc.div_(R)
                dcc.div_(R)
            if rev_complement:
                acc = acc.flip(1, 2)
            out[i:i + B] = acc.cpu().numpy()
            delta[i:i + B] = dcc.cpu().numpy()
    return (out, delta) if return_delta else out


def in_silico_mutagenesis(model, Xs, target=None, batch_size=4096, rev_complement=False, absolute=False,
                          return_logits=False):
    """In-silico mutagenesis in eval mode, float32 numpy (N,T,4,L) -- (N,4,L) for one `target`:
    row a at position p is logit(sequence with base a at p) - logit(sequence), 0 at the reference
    base; absolute=True gives the mutant logits themselves.  One device pass per batch
    (ExplaiNN.in_silico_mutagenesis) instead of 3L mutated copies through the model.

    Xs: (N,4,L) one-hot (numpy or tensor) or (N,L) uint8 base codes (0..3 = A,C,G,T, 4 = N).
    rev_complement=True runs the model on each sequence's reverse complement and maps rows and
    positions back (base a <-> 3-a, p <-> L-1-p), so that row a at p means "base a at p of the given
    strand".
    return_logits=True returns (result, logits), logits (N,T) float32: the logits of the strand the
    model ran on, all tasks whatever `target` says, the bits forward() gives."""
    Xs, codes, T, L, dev = _attribution_input(model, Xs, target)
    out = np.zeros((len(Xs), T, 4, L) if target is None else (len(Xs), 4, L), dtype=np.float32)
    all_logits = np.zeros((len(Xs), T), dtype=np.float32)
    with eval_mode(model), eval_pass(model):
        for i, xb in _batches(Xs, batch_size):
            xb, xin = _on_strand(xb.to(dev, non_blocking=True), codes, rev_complement)
            logits, delta = model.in_silico_mutagenesis(xin)
            if rev_complement:
                delta = delta.flip(2, 3)
            if absolute:
                delta = delta + logits[:, :, None, None]
            if target is not None:
                delta = delta[:, int(target)]
            out[i:i + xb.shape[0]] = delta.cpu().numpy()
            all_logits[i:i + xb.shape[0]] = logits.cpu().numpy()
    return (out, all_logits) if return_logits else out


def filter_importances(outs, final_weight, idxs, hit):
    """interpret.py:176-183 + 485-490: for each unit the (T, n) importances outs*weight of the
    well-predicted sequences with at least one position above the unit's threshold.  `hit` is
    filter_pwms' (N,U) matrix (it replaces `np.where(acts > threshold)[0]` on the dense array)."""
    res = []
    for u in range(outs.shape[1]):
        sel = np.intersect1d(idxs, np.where(hit[:, u])[0])
        imps = np.array([np.multiply(outs[sel, u], final_weight[t, u])
                         for t in range(final_weight.shape[0])])
        res.append((sel, imps))
    return res


def format_jaspar(pfm_u, matrix_id, name):
    """One motif in the JASPAR text layout Bio.motifs writes for `format(motif, "jaspar")`
    (interpret.py:228-231).  biopython is not available in this image, so the layout follows its
    published format ('>id name' then 'A [ %6.2f ...]' rows) and is not pinned by a fixture."""
    lines = [">%s %s\n" % (matrix_id, name)]
    for a, letter in enumerate("ACGT"):
        lines.append("%s [%s]\n" % (letter, " ".join("%6.2f" % v for v in pfm_u[:, a])))
    return "".join(lines)


def interpret(exp_model, seqs, labels, name, output_dir="./", batch_size=100, rev_complement=False,
              input_data=None, sites=False, meme=False):
    """The filter-level part of interpret.py's main (interpret.py:128-235): output-layer weights,
    filter importances and one JASPAR motif per filter, written under output_dir.  sites=True also
    writes thresholds.tsv and sites/filter<u>.fa (write_sites); meme=True also writes motifs/filters.meme,
    the filters that have a site as one MEME file (motifs.write_meme), for an external Tomtom."""
    import pandas as pd
    if input_data is None:
        input_data = "binary" if np.unique(labels[:, 0]).size == 2 else "linear"
    os.makedirs(os.path.join(output_dir, "motifs"), exist_ok=True)
    weights = exp_model.final.weight.detach().cpu().numpy()
    U = weights.shape[1]
    rows = [["filter%d" % u] + w.tolist() for u, w in enumerate(weights.T)]
    pd.DataFrame(rows, columns=["filter"] + list(range(weights.shape[0]))).to_csv(
        os.path.join(output_dir, "output-layer-weights.tsv"), sep="\t", index=False)
    outs, preds = _get_outs_preds(exp_model, seqs, batch_size)
    idxs = _get_well_predicted_sequences(preds, labels, input_data, rev_complement)
    res = filter_pwms(exp_model, seqs, idxs, rev_complement, batch_size=max(batch_size, 4096))
    data = []
    for u, (_, imps) in enumerate(filter_importances(outs, weights, idxs, res["hit"])):
        data.extend([["filter%d" % u] + col.tolist() for col in imps.T])
    cols = ["filter"] + list(range(weights.shape[0]))
    df = pd.DataFrame(data, columns=cols)
    tsv = os.path.join(output_dir, "filter-importances.tsv")
    df.to_csv(tsv + ".gz", sep="\t", index=False, compression="gzip")
    df = df.groupby(["filter"]).median().sort_values([cols[-1]], ascending=False)
    df.reset_index(inplace=True)
    df.to_csv(tsv, sep="\t", index=False)
    for u in range(U):
        with open(os.path.join(output_dir, "motifs", "filter%d.jaspar" % u), "wt") as fh:
            if res["nsites"][u] > 0:          # the reference leaves the file empty when no site
                fh.write(format_jaspar(res["pfm"][u], "filter%d" % u, name))
    if meme:
        from .motifs import write_meme
        kept = [u for u in range(U) if res["nsites"][u] > 0]
        write_meme(os.path.join(output_dir, "motifs", "filters.meme"),
                   [("filter%d" % u, name, res["pfm"][u]) for u in kept], [int(res["nsites"][u]) for u in kept])
    if sites:
        k = exp_model._options["kernel_size"]
        lists = filter_site_list(exp_model, seqs, idxs, res["thresholds"], rev_complement)
        write_sites(output_dir, lists, [site_kmers(seqs, lst, k, rev_complement) for lst in lists],
                    res["thresholds"])
    return res


def main(argv=None):
    from .predict import _load_model
    from .train import _get_seqs_labels_ids
    ap = argparse.ArgumentParser(description="Filter PWMs and importances of a trained ExplaiNN "
                                             "(device-side counterpart of the reference's interpret.py)")
    ap.add_argument("model_file")
    ap.add_argument("training_file")
    ap.add_argument("-b", "--batch-size", type=int, default=100)
    ap.add_argument("-d", "--debugging", action="store_true")
    ap.add_argument("-n", "--name", required=True)
    ap.add_argument("-o", "--output-dir", default="./")
    ap.add_argument("-r", "--rev-complement", action="store_true")
    ap.add_argument("-t", "--time-me", action="store_true")
    ap.add_argument("--sites", action="store_true",
                    help="also write thresholds.tsv and sites/filter<u>.fa (one k-mer per site)")
    ap.add_argument("--meme", action="store_true",
                    help="also write motifs/filters.meme (every filter with a site, MEME format)")
    args = ap.parse_args(argv)
    t0 = time.time()
    seqs, labels, _ = _get_seqs_labels_ids(args.training_file, args.debugging, args.rev_complement)
    model = _load_model(args.model_file)
    interpret(model, seqs, labels, args.name, args.output_dir, args.batch_size, args.rev_complement,
              sites=args.sites, meme=args.meme)
    if args.time_me:
        with open(os.path.join(args.output_dir, "time-interpret.py.txt"), "wt") as fh:
            fh.write("%.2f seconds" % (time.time() - t0))


if __name__ == "__main__":
    main()
