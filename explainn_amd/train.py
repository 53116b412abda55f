"""Training entry points (reference: explainn/train.py).

`_train` keeps the reference signature (train.py:304-307) and wiring: build `ExplaiNN`, loss,
metrics, Adam, optional transfer learning of the first filters, then `Trainer.train_and_validate`.
`main` is a thin argparse CLI with the reference's option names (the reference uses click +
click_option_group, which is not a dependency here).
"""
import argparse
import math
import os
import shutil
import time

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

from .architectures import ExplaiNN, get_loss, get_metrics, get_optimizer
from .selene import Trainer
from .sequence import one_hot_encode_many, rc_one_hot_encoding_many


def _get_seqs_labels_ids(tsv_file, debugging=False, reverse_complement=False):
    """train.py:266-284: headerless TSV `id <tab> sequence <tab> y0 [<tab> y1 ...]`."""
    import pandas as pd
    df = pd.read_csv(tsv_file, sep="\t", header=None)
    ids = df.pop(0).values
    seqs = one_hot_encode_many(df.pop(1).values)
    labels = df.values
    if reverse_complement:
        seqs = np.append(seqs, rc_one_hot_encoding_many(seqs), axis=0)
        labels = np.append(labels, labels, axis=0)
        ids = np.append(ids, ids, axis=0)
    if debugging:
        return seqs[:1000], labels[:1000], ids[:1000]
    return seqs, labels, ids


def _get_codes_loader(tsv_file, batch_size=100, shuffle=False, debugging=False,
                      reverse_complement=False, device=None):
    """The same data set as `_get_seqs_labels_ids` + `_get_data_loader` (train.py:266-295), kept as
    (N,L) base codes instead of a float64 (N,4,L) one-hot: vectorised parsing, reverse complement
    generated per batch, pinned staging + asynchronous copies (loader.CodesLoader).  Batches have
    the reference loader's order and contents; the model treats codes and one-hot identically."""
    from .loader import CodesLoader, read_tsv_codes
    codes, labels, _ = read_tsv_codes(tsv_file, debugging)
    # --debugging: the reference cuts to 1000 items AFTER the reverse-complement doubling
    loader = CodesLoader(codes, labels, batch_size, shuffle, reverse_complement, device,
                         limit=1000 if debugging else None)
    return loader, codes, labels


def _avoid_single_sample_batch(n, batch_size):
    """train.py:297-302: shrink the batch until the last batch is not a single sample
    (BatchNorm raises on one value per channel in train mode)."""
    while batch_size > 1 and n % batch_size == 1:
        batch_size -= 1
    return batch_size


class _BatchedTensorDataset(TensorDataset):
    """TensorDataset whose batches are cut with one index op per tensor (`__getitems__`, which
    torch's DataLoader prefers when present) instead of batch_size `__getitem__` calls plus a
    collate: 0.02 ms instead of 0.25 ms per batch of 100 -- at the reference's default shape the
    stock loader cost more host time than the whole training step takes on the GPU."""

    def __getitems__(self, indices):
        idx = torch.as_tensor(indices)
        return tuple(t[idx] for t in self.tensors)


def _already_batched(batch):
    return batch


def _get_data_loader(seqs, labels, batch_size=100, shuffle=False):
    """train.py:286-295: a torch DataLoader over (sequences, labels) -- same sampler, same batch
    order and contents as the reference's, cut batch-wise (see _BatchedTensorDataset)."""
    dataset = _BatchedTensorDataset(torch.Tensor(seqs), torch.Tensor(labels))
    return DataLoader(dataset, _avoid_single_sample_batch(len(dataset), batch_size),
                      shuffle=shuffle, collate_fn=_already_batched)


def _train(sequence_length, n_features, data_loaders, input_data, steps_per_epoch, cnn_units=100,
           kernel_size=19, lr=0.003, max_epochs=100, patience=10, cpu_threads=1, output_dir="./",
           filter_weights=[], freeze=False, checkpoint_resume=None, sync_batchnorm=False,
           device_metrics=False):
    """train.py:304-342.  sync_batchnorm: BatchNorm statistics of the whole batch across
    data-parallel ranks (selene.Trainer's keyword; off = per-shard, the reference's DDP semantics).
    device_metrics: validation metrics computed on the device (selene.Trainer's keyword; off = the
    reference's scikit-learn / scipy callables on host copies)."""
    freeze_top_n_filters = 0
    exp_model = ExplaiNN(cnn_units, kernel_size, sequence_length, n_features)
    loss_criterion = get_loss(input_data=input_data)
    metrics = get_metrics(input_data=input_data)
    optimizer = get_optimizer(exp_model.parameters(), lr)
    if len(filter_weights) > 0:
        # Transfer learning, statement for statement what train.py:316-324 does -- including its
        # consequence: the optimiser above was built from the ORIGINAL `linears[0].weight`
        # Parameter, and the re-assignment below puts a NEW Parameter (same storage) into the
        # model, so Adam keeps a Parameter that never receives a gradient again and the filter
        # bank stays at `filter_weights` for the whole run, `freeze` or not; every other parameter
        # trains normally (fixture tests/golden/transfer.npz, generated by the reference's own
        # `_train`).  Fewer filters than units is an IndexError there and here.
        finetuning_filter_weights = exp_model.linears[0].weight.data
        for i in range(finetuning_filter_weights.shape[0]):
            finetuning_filter_weights[i] = torch.as_tensor(filter_weights[i])
            if freeze:
                freeze_top_n_filters += 1
        finetuning_filter_weights.requires_grad = True
        exp_model.linears[0].weight = nn.Parameter(finetuning_filter_weights)
    trainer = Trainer(
        exp_model, data_loaders, loss_criterion, metrics, optimizer,
        max_steps=steps_per_epoch * max_epochs, patience=steps_per_epoch * patience,
        report_stats_every_n_steps=steps_per_epoch, output_dir=output_dir,
        cpu_n_threads=cpu_threads, use_cuda=torch.cuda.is_available(),
        checkpoint_resume=checkpoint_resume, freeze_top_n_filters=freeze_top_n_filters,
        sync_batchnorm=sync_batchnorm, device_metrics=device_metrics)
    trainer.train_and_validate()
    return trainer


def _train_bank(n_models, sequence_length, n_features, data_loaders, input_data, steps_per_epoch,
                cnn_units=100, kernel_size=19, lr=0.003, max_epochs=5, patience=10, cpu_threads=1,
                output_dir="./"):
    """The `--initialize` short runs as ONE bank run (selene.BankTrainer): n_models independently
    initialised models trained on the same batches, leaving `output_dir/init.<g>/` as the
    sequential runs do."""
    from .architectures import ExplaiNNBank
    from .selene import BankTrainer
    bank = ExplaiNNBank(n_models, cnn_units, kernel_size, sequence_length, n_features)
    trainer = BankTrainer(
        bank, data_loaders, input_data, get_metrics(input_data=input_data),
        get_optimizer(bank.parameters(), lr), max_steps=steps_per_epoch * max_epochs,
        patience=steps_per_epoch * patience, report_stats_every_n_steps=steps_per_epoch,
        output_dir=output_dir, cpu_n_threads=cpu_threads)
    trainer.train_and_validate()
    return trainer


def _load_filter_weights(path):
    """train.py:183-195: a file of pre-trained filters `{id: (k,4) array}` -> (ids, [(4,k) tensors]).
    `.npz` archives are read directly; the reference's pickles go through an unpickler that only
    admits numpy arrays/dtypes and plain containers (nothing else in the file can execute)."""
    import pickle
    if path.endswith(".npz"):
        z = np.load(path, allow_pickle=False)
        w = {k: z[k] for k in z.files}
    else:
        class _ArraysOnly(pickle.Unpickler):
            # protocol 5 (pickle.HIGHEST_PROTOCOL, what interpret.py:162 writes) serialises
            # contiguous and Fortran-order arrays through _frombuffer (array-from-bytes, nothing more)
            _ok = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
                   ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer"),
                   ("numpy", "ndarray"), ("numpy", "dtype"), ("collections", "OrderedDict")}

            def find_class(self, module, name):
                if (module, name) in self._ok:
                    return super().find_class(module, name)
                raise pickle.UnpicklingError("%s.%s is not allowed in a filter-weights file" % (module, name))
        import gzip
        with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as fh:
            w = _ArraysOnly(fh).load()
    ids, weights = [], []
    for k, v in w.items():
        ids.append(k if isinstance(k, str) else ";".join(k))
        weights.append(torch.tensor(np.asarray(v).T))
    return ids, weights


def main(argv=None):
    """train.py:151-264: load TSVs, pick the best of `--initialize` short runs, train."""
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("training_file"); ap.add_argument("validation_file")
    ap.add_argument("-b", "--batch-size", type=int, default=100)
    ap.add_argument("-c", "--cpu-threads", type=int, default=1)
    ap.add_argument("-d", "--debugging", action="store_true")
    ap.add_argument("-i", "--initialize", type=int, default=1)
    ap.add_argument("-o", "--output-dir", default="./")
    ap.add_argument("-r", "--rev-complement", action="store_true")
    ap.add_argument("-t", "--time-me", action="store_true")
    ap.add_argument("--cnn-units", type=int, default=100)
    ap.add_argument("--kernel-size", type=int, default=19)
    ap.add_argument("--lr", type=float, default=0.003)
    ap.add_argument("--max-epochs", type=int, default=100)
    ap.add_argument("--patience", type=int, default=10)
    ap.add_argument("--filter-weights", action="append", default=[])
    ap.add_argument("--freeze", action="store_true")
    ap.add_argument("--sync-batchnorm", action="store_true",
                    help="data-parallel runs: BatchNorm statistics of the whole batch across ranks")
    ap.add_argument("--device-metrics", action="store_true",
                    help="compute the validation metrics on the GPU instead of with scikit-learn / scipy")
    ap.add_argument("--bank", action="store_true",
                    help="run the --initialize short runs as ONE model bank (all initialisations in "
                         "one fused step per batch; needs a GPU).  The members of a bank see the same "
                         "batch order; sequential runs each draw their own shuffle")
    args = ap.parse_args(argv)
    if args.bank and args.filter_weights:
        ap.error("--bank cannot be combined with --filter-weights (transfer learning)")
    if args.bank and args.sync_batchnorm:
        ap.error("--bank cannot be combined with --sync-batchnorm")
    import pandas as pd
    start = time.time()
    os.makedirs(args.output_dir, exist_ok=True)
    dev = "cuda" if torch.cuda.is_available() else None
    tr, c_tr, l_tr = _get_codes_loader(args.training_file, args.batch_size, True, args.debugging,
                                       args.rev_complement, dev)
    va, _, _ = _get_codes_loader(args.validation_file, args.batch_size, True, args.debugging,
                                 args.rev_complement, dev)
    loaders = {"train": tr, "validation": va}
    L, T = c_tr.shape[1], l_tr.shape[1]
    input_data = "binary" if np.unique(l_tr[:, 0]).size == 2 else "linear"
    spe = math.ceil(len(loaders["train"].dataset) / loaders["train"].batch_size)
    filter_ids, filter_weights = [], []
    for f in args.filter_weights:                     # train.py:183-203
        ids, ws = _load_filter_weights(f)
        filter_ids += ids; filter_weights += ws
    if filter_ids:
        with open(os.path.join(args.output_dir, "filter-ids-from-pre-training-step.txt"), "wt") as fh:
            fh.write("\n".join(filter_ids))
    best_loss, best_model = None, None
    if args.bank and not all(os.path.isdir(os.path.join(args.output_dir, "init.%d" % i))
                             for i in range(args.initialize)):
        _train_bank(args.initialize, L, T, loaders, input_data, spe, args.cnn_units, args.kernel_size,
                    args.lr, 5, args.patience, args.cpu_threads, args.output_dir)
    for i in range(args.initialize):
        d = os.path.join(args.output_dir, "init.%d" % i)
        if not os.path.isdir(d):
            os.makedirs(d)
            _train(L, T, loaders, input_data, spe, args.cnn_units, args.kernel_size, args.lr, 5,
                   args.patience, args.cpu_threads, d, filter_weights, args.freeze,
                   sync_batchnorm=args.sync_batchnorm, device_metrics=args.device_metrics)
        loss = pd.read_csv(os.path.join(d, "validation.txt"), sep="\t").loss.min()
        if best_model is None or loss < best_loss:
            best_loss, best_model = loss, os.path.join(d, "best_model.pth.tar")
    shutil.copy(best_model, args.output_dir)
    _train(L, T, loaders, input_data, spe, args.cnn_units, args.kernel_size, args.lr,
           args.max_epochs, args.patience, args.cpu_threads, args.output_dir, filter_weights,
           args.freeze, best_model, sync_batchnorm=args.sync_batchnorm,
           device_metrics=args.device_metrics)
    if args.time_me:
        with open(os.path.join(args.output_dir, "time-train.py.txt"), "wt") as fh:
            fh.write("%.2f seconds" % (time.time() - start))


if __name__ == "__main__":
    main()
