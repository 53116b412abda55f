"""Training harness around the hot loop (reference: explainn/selene/__init__.py, `Trainer`).

Same constructor arguments, same step order (selene/__init__.py:283-295: train mode, forward, loss,
zero_grad, backward, optimiser step, loss.item()), same validation / early stopping / best-model
checkpoint contents and the same `train.txt`, `validation.txt`, `selene.log` outputs (which
train.py:240-241 re-reads).  The difference is what runs inside a step: when the criterion is one
of the two losses `get_loss` returns and the model is `explainn_amd.ExplaiNN`, the whole
forward + loss + backward is ONE C-ABI call (`StepEngine`), gradients land in a flat buffer, and
with torch.distributed initialised that buffer is all-reduced once per step.
"""
import contextlib
import copy
import logging
import os
import sys
from time import time

import numpy as np
import torch

from .architectures import ExplaiNN
from .engine import StepEngine
from . import parallel

logger = logging.getLogger("selene")


class Trainer(object):
    """Trains a model for `max_steps` mini-batches, validating every
    `report_stats_every_n_steps` and stopping early after `patience` steps without improvement."""

    def __init__(self, model, data_loaders, loss_criterion, metrics, optimizer, max_steps=128000,
                 patience=32000, report_stats_every_n_steps=1000, output_dir="./",
                 cpu_n_threads=1, use_cuda=False, checkpoint_resume=None, freeze_top_n_filters=0,
                 logging_verbosity=2, sync_batchnorm=False, device_metrics=False):
        self.model = model
        # opt-in: validation predictions and targets stay on the device and the
        # metrics are computed there (explainn_amd.metrics) instead of by the `metrics` callables on
        # host copies; the names in `metrics` say which pair
        self.device_metrics = bool(device_metrics)
        if self.device_metrics:
            from . import metrics as _device_metrics
            self._device_metric_kind = _device_metrics.kind_of(metrics.keys())
        # opt-in sync-BN: BatchNorm statistics of the whole batch across ranks; the
        # steps then leave the global gradients on every rank and no gradient all-reduce runs
        self.sync_batchnorm = bool(sync_batchnorm)
        if self.sync_batchnorm:
            parallel.sync_batchnorm(model, parallel.ProcessGroupReducer())
        self.data_loaders = data_loaders
        self.criterion = loss_criterion
        self.metrics = metrics
        self.optimizer = optimizer
        self.max_steps = max_steps
        self.patience = patience
        self.nth_step_report_stats = report_stats_every_n_steps
        torch.set_num_threads(cpu_n_threads)
        os.makedirs(output_dir, exist_ok=True)
        self.output_dir = output_dir
        self.freeze_top_n_filters = freeze_top_n_filters
        self.logger = selene_logger(self.output_dir, logging_verbosity)
        self.use_cuda = use_cuda
        if self.use_cuda:
            self.model.cuda()
            self.criterion.cuda()
            self.logger.debug("Set modules to use CUDA")
        self._data_iterators = {k: [] for k in self.data_loaders.keys()}
        self._engine = None
        self._grad_sync = None
        self._init_train()
        self._init_validate()
        if checkpoint_resume is not None:
            self._load_checkpoint(checkpoint_resume)

    # ---- bookkeeping (selene/__init__.py:191-221) ----
    def _init_train(self):
        self._start_step = 1
        self._train_logger = metrics_logger("train", self.output_dir)
        self.logger.info("Training metrics: loss")
        self._train_logger.log(10, "loss")
        self._time_per_step = []
        self._train_loss = []

    def _init_validate(self):
        self._min_loss = float("inf")
        self._best_step = 1
        self._validation_logger = metrics_logger("validation", self.output_dir)
        names = ["loss"] + [x for x in self.metrics.keys()]
        self.logger.info("Validation metrics: " + ", ".join(names))
        self._validation_logger.log(10, "\t".join(names))

    def _load_checkpoint(self, checkpoint_resume):
        checkpoint = _load_checkpoint_file(checkpoint_resume)
        self.model.load_state_dict(checkpoint["state_dict"])
        self._start_step = checkpoint["step"]
        self._min_loss = checkpoint["min_loss"]
        self._best_step = checkpoint["step"]
        self.optimizer.load_state_dict(checkpoint["optimizer"])
        if self.use_cuda:
            for state in self.optimizer.state.values():
                for k, v in state.items():
                    # the step counter stays on the host (torch's Adam requires it there unless
                    # capturable; the reference's blanket .cuda() predates that check)
                    if isinstance(v, torch.Tensor) and k != "step":
                        state[k] = v.cuda()
        self.logger.info("Resuming from checkpoint: step %s, min loss %s" % (
            self._start_step, self._min_loss))

    def _get_batch(self, which_data):
        """Next mini-batch; the iterator restarts when exhausted (selene/__init__.py:223-246)."""
        t0 = time()
        try:
            batch = next(self._data_iterators[which_data])
        except (StopIteration, TypeError):
            self._data_iterators[which_data] = iter(self.data_loaders[which_data])
            batch = next(self._data_iterators[which_data])
        self.logger.debug("[BATCH] Time to sample batch: %s s." % (time() - t0))
        return batch

    # ---- the loop (selene/__init__.py:248-308) ----
    def train_and_validate(self):
        hook = None
        if self.freeze_top_n_filters > 0 and not self._fused_step_available():
            n = self.freeze_top_n_filters

            def _mask(grad):
                keep = torch.ones_like(grad)
                keep[:n] = 0
                return grad * keep
            hook = self.model.linears[0].weight.register_hook(_mask)
        for step in range(self._start_step, self.max_steps + 1):
            self.step = step
            self.train()
            if self.step % self.nth_step_report_stats == 0:
                self.validate()
            if self.step >= self._best_step + self.patience:
                self.logger.info("Early stopping: stop training!")
                break
        if hook is not None:
            hook.remove()
        if self.use_cuda and isinstance(self.model, ExplaiNN) and self.model.validate_input:
            self._check_input_flags()
        self.logger.handlers.clear()
        self._train_logger.handlers.clear()
        self._validation_logger.handlers.clear()

    def _fused_step_available(self):
        return (isinstance(self.model, ExplaiNN) and self.use_cuda and
                type(self.criterion) in (torch.nn.BCEWithLogitsLoss, torch.nn.MSELoss) and
                getattr(self.criterion, "reduction", "mean") == "mean" and
                getattr(self.criterion, "weight", None) is None and
                getattr(self.criterion, "pos_weight", None) is None)

    def _fused_engine(self, batch):
        if self._engine is None:
            kind = "binary" if isinstance(self.criterion, torch.nn.BCEWithLogitsLoss) else "linear"
            self._engine = StepEngine(self.model, batch, loss=kind)
            if parallel.world() > 1:
                parallel.broadcast_parameters(self.model)
            if parallel.world() > 1 and not self.sync_batchnorm:
                self._grad_sync = parallel.GradAllReduce(self._engine.flat_grad,
                                                         split=self._engine.conv_grad_elements)
        return self._engine

    def train(self):
        """One optimisation step on one mini-batch; returns nothing, logs like the reference."""
        t_i = time()
        if not self.model.training:          # selene/__init__.py:283 (a 17-module walk when repeated)
            self.model.train()
        inputs, targets = self._get_batch("train")
        if self.use_cuda:
            inputs = inputs.cuda()
            targets = targets.cuda()
        global_batch = inputs.shape[0]
        if parallel.world() > 1:
            inputs, targets = parallel.shard_batch(inputs, targets)
        if self._fused_step_available():
            eng = self._fused_engine(inputs.shape[0])
            # parameters are re-pointed only outside the loop (train.py:318-324 re-assigns the filter
            # bank before training; the optimiser updates in place): rebuild the pointer table when
            # the first parameter moved, and every 64th step as a safety net
            w0 = self.model.linears[0].weight
            if self.step % 64 == 1 or getattr(self, "_w0_ptr", None) != w0.data_ptr():
                eng.refresh_params()
                self._w0_ptr = w0.data_ptr()
            if inputs.dtype != torch.uint8:           # base codes (loader.CodesLoader) go in as they are
                inputs = inputs.float()
            _, loss = eng.step(inputs.contiguous(), targets.float().contiguous(),
                               seed=int(torch.randint(0, 2 ** 62, (1,)).item()),
                               freeze_top_n_filters=self.freeze_top_n_filters,
                               global_batch=global_batch if self.sync_batchnorm else None)
            if self._grad_sync is not None:
                self._grad_sync()       # one all-reduce of the flat buffer
            eng.attach_grads()
            self.optimizer.step()
            # The reference reads loss.item() here, stalling the host on the device every step; the
            # values are only consumed when the running mean is reported, so the fused path keeps
            # them on the device until then (or until 256 have piled up) and the host runs ahead.
            loss_value = loss.clone()
            # the device-side input validation flag is sticky: reading it (a second device-to-host
            # round trip) on the first steps and then every 64th reports a non-one-hot input without
            # paying for the check on every step; train_and_validate() reads it once more at the end
            if self.model.validate_input and (self.step <= 3 or self.step % 64 == 0):
                self._check_input_flags()
        else:
            if parallel.world() > 1 and self.model.grad_sync is None and not self.sync_batchnorm:
                # the autograd path of a sharded run (weighted / custom criterion): same start and
                # the same averaged gradients as the fused path, one all-reduce per backward
                parallel.broadcast_parameters(self.model)
                self.model.grad_sync = parallel.average_gradients
            if parallel.world() > 1 and self.sync_batchnorm and not getattr(self, "_synced_start", False):
                parallel.broadcast_parameters(self.model)
                self._synced_start = True
            predictions = self.model(inputs)
            loss = self.criterion(predictions, targets)
            self.optimizer.zero_grad()
            loss.backward()
            self.optimizer.step()
            loss_value = loss.item()
        self._train_loss.append(loss_value)
        if len(self._train_loss) % 256 == 0:
            self._settle_train_loss()
        self._time_per_step.append(time() - t_i)
        if self.step > 0 and self.step % self.nth_step_report_stats == 0:
            self._settle_train_loss()
            self.logger.info("[STEP %d] average number of steps per second: %s" % (
                self.step, 1. / np.average(self._time_per_step)))
            self.logger.info("Training loss: %s" % np.average(self._train_loss))
            self._train_logger.log(10, np.average(self._train_loss))
            self._time_per_step = []
            self._train_loss = []

    def _settle_train_loss(self):
        """Turn the loss values still held as device tensors into floats (one transfer)."""
        pending = [i for i, v in enumerate(self._train_loss) if torch.is_tensor(v)]
        if pending:
            vals = torch.cat([self._train_loss[i].reshape(1) for i in pending]).tolist()
            for i, v in zip(pending, vals):
                self._train_loss[i] = v

    def _check_input_flags(self):
        if self.model.input_flags() & 1:
            raise ValueError("input is not one-hot (see explainn_amd.ExplaiNN.forward)")

    def _evaluate_on_data(self, which_data):
        """Average loss + all predictions/targets over a data set (selene/__init__.py:310-342)."""
        self.model.eval()
        batch_losses, all_predictions, all_targets = [], [], []
        cache = self.model.eval_cache() if isinstance(self.model, ExplaiNN) else contextlib.nullcontext()
        with cache:
            out = self._evaluate_batches(which_data, batch_losses, all_predictions, all_targets)
        if self.use_cuda and isinstance(self.model, ExplaiNN) and self.model.validate_input:
            self._check_input_flags()
        return out

    def _evaluate_batches(self, which_data, batch_losses, all_predictions, all_targets):
        for inputs, targets in iter(self.data_loaders[which_data]):
            # a device-resident loader (loader.CodesLoader) yields views of a staging ring: cloned
            # on the device and brought to the host ONCE after the loop; host batches are kept as is
            all_targets.append(targets.data.clone() if targets.is_cuda else targets.data)
            if self.use_cuda:
                inputs = inputs.cuda()
                targets = targets.cuda()
            with torch.no_grad():
                predictions = self.model(inputs)
                # kept on the device; the reference's per-batch .cpu()/.item() reads are done once,
                # after the loop
                batch_losses.append(self.criterion(predictions, targets).reshape(1))
                all_predictions.append(predictions.data)
        if self.device_metrics:
            return self._on_device(batch_losses, all_predictions, all_targets)
        losses = torch.cat(batch_losses).tolist() if batch_losses else []
        preds = torch.cat(all_predictions).cpu().numpy() if all_predictions else np.zeros((0, 0))
        tgts = torch.cat(all_targets).cpu().numpy() if all_targets else np.zeros((0, 0))
        return (np.average(losses), preds, tgts)

    def _on_device(self, batch_losses, all_predictions, all_targets):
        """device_metrics: (batch losses, predictions, targets) as device tensors, nothing read."""
        if not all_predictions:
            raise ValueError("device_metrics: the data loader gave no batch")
        dev = all_predictions[0].device
        if dev.type != "cuda":
            raise RuntimeError("device_metrics needs the model on a HIP device (use_cuda=True). "
                               "There is no CPU fallback.")
        return (torch.cat(batch_losses), torch.cat(all_predictions),
                torch.cat([t.to(dev) for t in all_targets]))

    def _device_scores(self, batch_losses, predictions, targets):
        """Loss average and both metrics of the pair from ONE device-to-host transfer.  The average is
        numpy's over the same float32 batch losses as the host path takes, hence the same value."""
        from . import metrics as dm
        pair = dm._run(self._device_metric_kind, targets.reshape(-1), predictions.reshape(-1), False)
        vals = dm.read(pair[0], pair[1], dm._wrap(batch_losses.to(torch.float64), pair[0]._call, 0))
        scores = dict(zip(dm.NAMES[self._device_metric_kind], vals[:2]))
        return np.average(vals[2]), {name: scores[name] for name in self.metrics}

    def validate(self):
        """Validation metrics on flattened predictions; best model -> best_model.pth.tar
        (selene/__init__.py:344-391)."""
        validation_loss, all_predictions, all_targets = self._evaluate_on_data("validation")
        if self.device_metrics:
            validation_loss, valid_scores = self._device_scores(validation_loss, all_predictions, all_targets)
        self.logger.info("Validation loss: %s" % validation_loss)
        valid_scores = valid_scores if self.device_metrics else {}
        for metric in ({} if self.device_metrics else self.metrics):
            score = self.metrics[metric](all_targets.flatten(), all_predictions.flatten())
            valid_scores[metric] = score if isinstance(score, float) else score[0]
        for name, score in valid_scores.items():
            self.logger.info("Validation %s: %s" % (name, score))
        self._validation_metrics = valid_scores
        if validation_loss < self._min_loss:
            self._min_loss = validation_loss
            self._best_step = int(self.step)
            if parallel.rank() == 0:
                model = copy.deepcopy(self.model)
                self._save_checkpoint({
                    "step": self._best_step,
                    "arch": model.__class__.__name__,
                    "options": model._options,
                    "state_dict": model.state_dict(),
                    "min_loss": self._min_loss,
                    "optimizer": copy.deepcopy(self.optimizer.state_dict()),
                })
                self.logger.info("Updating `best_model.pth.tar`")
        self._validation_logger.log(
            10, "\t".join(map(str, [validation_loss] + list(valid_scores.values()))))

    def _save_checkpoint(self, state):
        self.logger.debug("[TRAIN] %s: Saving model state to file." % state["step"])
        torch.save(state, os.path.join(self.output_dir, "best_model.pth.tar"))


class BankRecord:
    """Per-member bookkeeping of a bank run, kept apart from the compute: fed with the vector of G
    validation losses of every report, it holds each member's `_min_loss` / `_best_step` exactly as
    Trainer.validate does (strict `<`: a tie or a NaN is no improvement) and says which members'
    files are to be written.  A member that went `patience` steps without improving is final: it
    keeps stepping with the bank but its files are not touched again."""

    def __init__(self, n_models, patience):
        self.patience = patience
        self.min_loss = [float("inf")] * n_models
        self.best_step = [1] * n_models
        self.final = [False] * n_models

    def report(self, step, losses):
        """Returns (live, improved): the members whose files still get this report's lines (those not
        final before it) and, among them, the ones that improved (their checkpoints are due); then
        applies the early-stopping rule of Trainer.train_and_validate member by member."""
        live = [g for g, f in enumerate(self.final) if not f]
        improved = []
        for g in live:
            loss = float(losses[g])
            if loss < self.min_loss[g]:
                self.min_loss[g] = loss
                self.best_step[g] = int(step)
                improved.append(g)
        for g in live:
            if step >= self.best_step[g] + self.patience:
                self.final[g] = True
        return live, improved

    def done(self):
        return all(self.final)


class MemberFiles:
    """The `init.<g>/` directories of a bank run, written from plain values: `train.txt` and
    `validation.txt` in the column layout of metrics_logger (a header line, then one line per
    report) and `best_model.pth.tar` with exactly the keys Trainer.validate writes."""

    def __init__(self, output_dir, n_models, metric_names):
        self.dirs = [os.path.join(output_dir, "init.%d" % g) for g in range(n_models)]
        for d in self.dirs:
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "train.txt"), "wt") as fh:
                fh.write("loss\n")
            with open(os.path.join(d, "validation.txt"), "wt") as fh:
                fh.write("\t".join(["loss"] + list(metric_names)) + "\n")

    def _append(self, g, name, values):
        with open(os.path.join(self.dirs[g], name), "at") as fh:
            fh.write("\t".join(map(str, values)) + "\n")

    def train(self, g, loss):
        self._append(g, "train.txt", [loss])

    def validation(self, g, loss, scores):
        self._append(g, "validation.txt", [loss] + list(scores))

    def checkpoint(self, g, step, options, state_dict, min_loss, optimizer_state):
        torch.save({"step": int(step), "arch": "ExplaiNN", "options": dict(options),
                    "state_dict": state_dict, "min_loss": min_loss, "optimizer": optimizer_state},
                   os.path.join(self.dirs[g], "best_model.pth.tar"))


class BankTrainer(object):
    """Trainer for an ExplaiNNBank: every step is ONE fused step of all G members on the same batch
    (StepEngine on the bank, one optimiser over the stacked parameters), validation is one eval pass
    per batch for all members, and every member gets the files a Trainer run of its own would leave,
    under `<output_dir>/init.<g>/` (MemberFiles), whenever THAT member improves.  Stops at max_steps
    or when every member ran out of patience (BankRecord).  Members see the same batches in the same
    order.  input_data: "binary" (BCE with logits) or anything else (MSE), as get_loss takes it."""

    def __init__(self, bank, data_loaders, input_data, metrics, optimizer, max_steps=128000,
                 patience=32000, report_stats_every_n_steps=1000, output_dir="./", cpu_n_threads=1,
                 freeze_top_n_filters=0, logging_verbosity=2):
        from .architectures import ExplaiNNBank
        if not isinstance(bank, ExplaiNNBank):
            raise TypeError("BankTrainer trains an explainn_amd.ExplaiNNBank")
        self.model = bank
        self.data_loaders = data_loaders
        self.kind = "binary" if input_data == "binary" else "linear"
        self.metrics = metrics
        self.optimizer = optimizer
        self.max_steps = max_steps
        self.nth_step_report_stats = report_stats_every_n_steps
        self.freeze_top_n_filters = freeze_top_n_filters
        torch.set_num_threads(cpu_n_threads)
        os.makedirs(output_dir, exist_ok=True)
        self.output_dir = output_dir
        self.logger = selene_logger(output_dir, logging_verbosity)
        self.model.cuda()
        self.record = BankRecord(bank._groups, patience)
        self.files = MemberFiles(output_dir, bank._groups, list(metrics.keys()))
        self._data_iterators = {k: [] for k in data_loaders}
        self._engine = None
        self._train_loss = []
        self.step = 0

    _get_batch = Trainer._get_batch

    def train_and_validate(self):
        for step in range(1, self.max_steps + 1):
            self.step = step
            self.train()
            if step % self.nth_step_report_stats == 0:
                self.validate()
            if self.record.done():
                self.logger.info("Early stopping: every member ran out of patience")
                break
        if self.model.validate_input and self.model.input_flags() & 1:
            raise ValueError("input is not one-hot (see explainn_amd.ExplaiNN.forward)")
        self.logger.handlers.clear()

    def train(self):
        if not self.model.training:
            self.model.train()
        inputs, targets = self._get_batch("train")
        inputs, targets = inputs.cuda(), targets.cuda().float().contiguous()
        if self._engine is None:
            self._engine = StepEngine(self.model, inputs.shape[0], loss=self.kind)
            self._engine.attach_grads()
        if inputs.dtype != torch.uint8:
            inputs = inputs.float()
        _, loss = self._engine.step(inputs.contiguous(), targets,
                                    seed=int(torch.randint(0, 2 ** 62, (1,)).item()),
                                    freeze_top_n_filters=self.freeze_top_n_filters)
        self.optimizer.step()
        self._train_loss.append(loss.clone())            # (G,), read when reported
        if self.step % self.nth_step_report_stats == 0:
            mean = torch.stack(self._train_loss).double().mean(dim=0).tolist()
            for g, v in enumerate(mean):
                if not self.record.final[g]:
                    self.files.train(g, v)
            self.logger.info("[STEP %d] training loss per member: %s" % (self.step, mean))
            self._train_loss = []

    def member_losses(self, predictions, targets):
        """(G,) losses of logits (B,G,T) against the shared targets (B,T): each the mean over the
        member's own B*T terms."""
        fn = (torch.nn.functional.binary_cross_entropy_with_logits if self.kind == "binary"
              else torch.nn.functional.mse_loss)
        t = targets[:, None, :].expand_as(predictions)
        return fn(predictions, t, reduction="none").mean(dim=(0, 2))

    def evaluate(self, which_data="validation"):
        """(per-member average of the batch losses (G,), predictions (N,G,T), targets (N,T)) from one
        eval pass per batch."""
        self.model.eval()
        losses, preds, tgts = [], [], []
        with self.model.eval_cache(), torch.no_grad():
            for inputs, targets in iter(self.data_loaders[which_data]):
                targets = targets.cuda().float()
                p = self.model(inputs.cuda())
                losses.append(self.member_losses(p, targets))
                preds.append(p.clone())
                tgts.append(targets.clone())
        if self.model.validate_input and self.model.input_flags() & 1:
            raise ValueError("input is not one-hot (see explainn_amd.ExplaiNN.forward)")
        # (float64, as Trainer's np.average of a list of floats: min_loss in the checkpoint is a numpy float64)
        loss = np.average(torch.stack(losses).cpu().numpy().astype(np.float64), axis=0)
        return loss, torch.cat(preds).cpu().numpy(), torch.cat(tgts).cpu().numpy()

    def validate(self):
        from .optim import member_state
        loss, preds, tgts = self.evaluate("validation")
        live, improved = self.record.report(self.step, loss)
        for g in live:
            scores = []
            for name, fn in self.metrics.items():
                score = fn(tgts.flatten(), preds[:, g].flatten())
                scores.append(score if isinstance(score, float) else score[0])
            self.files.validation(g, loss[g], scores)
            if g in improved:
                self.files.checkpoint(g, self.step, self.model._member_options(),
                                      self.model.member_state_dict(g), loss[g],
                                      member_state(self.optimizer, self.model, g))
                self.logger.info("Updating init.%d/best_model.pth.tar (loss %s)" % (g, loss[g]))


def _load_checkpoint_file(path):
    """Checkpoints hold tensors plus python/numpy scalars (`min_loss` is a numpy float in files the
    reference writes); allow exactly those under the safe unpickler."""
    import numpy.core.multiarray as _ma  # noqa: F401
    allow = [np.dtype, np.float64, np.float32]
    try:
        allow.append(np._core.multiarray.scalar)
    except AttributeError:
        allow.append(np.core.multiarray.scalar)
    try:
        allow.append(type(np.dtype(np.float64)))
    except Exception:
        pass
    with torch.serialization.safe_globals(allow):
        return torch.load(path, map_location="cpu", weights_only=True)


def selene_logger(logger_path="./", verbosity=2):
    """File + stdout logger named "selene" (selene/__init__.py:430-470); idempotent."""
    log = logging.getLogger("selene")
    if len(log.handlers):
        return log
    log.setLevel({0: logging.WARNING, 1: logging.INFO}.get(verbosity, logging.DEBUG))
    fh = logging.FileHandler(os.path.join(logger_path, "selene.log"))
    fh.setFormatter(logging.Formatter("%(asctime)s - %(levelname)s - %(message)s"))
    log.addHandler(fh)
    sh = logging.StreamHandler(sys.stdout)
    sh.setFormatter(logging.Formatter("%(asctime)s - %(message)s"))
    sh.setLevel(logging.INFO)
    log.addHandler(sh)
    return log


def metrics_logger(metric, logger_path="./", verbosity=2):
    """`<metric>.txt` value logger (selene/__init__.py:472-507); idempotent."""
    log = logging.getLogger(metric)
    if len(log.handlers):
        return log
    log.setLevel({0: logging.WARNING, 1: logging.INFO}.get(verbosity, logging.DEBUG))
    fh = logging.FileHandler(os.path.join(logger_path, "%s.txt" % metric))
    fh.setFormatter(logging.Formatter("%(message)s"))
    log.addHandler(fh)
    sh = logging.StreamHandler(sys.stdout)
    sh.setFormatter(logging.Formatter("%(asctime)s - %(message)s"))
    sh.setLevel(logging.INFO)
    log.addHandler(sh)
    return log


def freeze_top_n_filters(grad, freeze_top_n_filters=0, use_cuda=False):
    """Gradient hook of selene/__init__.py:509-515: zero the first n filters' gradient."""
    keep = torch.ones_like(grad)
    keep[:freeze_top_n_filters] = 0
    return grad * keep
