"""Supervised training / evaluation of a shifu Module on a dataset (reference shifu/runner/module_runner.py).

Scalars go to tensorboard when torch.utils.tensorboard is importable; otherwise to `<tensorboard_logdir>/scalars.jsonl`,
one JSON object per logged step: {"step": ..., "time": ..., "<run mode>/<loss name>": value, ...}."""
import json
import os
import time

import torch

from .utils import datetime_logdir, latest_logdir


class _JsonlWriter:
    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        self.path = os.path.join(logdir, "scalars.jsonl")
        self._step, self._row = None, {}

    def add_scalar(self, tag, value, global_step=None, walltime=None):
        if self._step is not None and global_step != self._step:
            self.flush()
        self._step = global_step
        self._row[tag] = float(value)

    def flush(self):
        if self._row:
            with open(self.path, "a") as f:
                f.write(json.dumps({"step": self._step, "time": time.time(), **self._row}) + "\n")
        self._step, self._row = None, {}

    def close(self):
        self.flush()


def _make_logger(tensorboard_logdir):
    try:
        from torch.utils.tensorboard import SummaryWriter
    except ImportError:
        return _JsonlWriter(tensorboard_logdir)
    return SummaryWriter(f"{tensorboard_logdir}/.tensorboard")


class ModuleRunner:
    """Fits (`train`) or scores (`play`) a Module on an iterable of (data, label) batches.  Checkpoints live in `logdir`,
    scalars under `tensorboard_logdir`; either may be None for a runner that is only used for `update`."""

    def __init__(self, model, lr=1e-4, weight_decay=1e-05, logdir=None, tensorboard_logdir=None, device='cuda:0',
                 optimizer_class=torch.optim.Adam):
        self.device = device
        self.model = model.to(device)
        self.lr, self.weight_decay = lr, weight_decay
        self.optimizer = optimizer_class(self.model.parameters(), lr=lr, weight_decay=weight_decay)
        self.logdir = logdir
        self.logger = None if tensorboard_logdir is None else _make_logger(tensorboard_logdir)
        self._began, self._items = time.time(), 0

    def update(self, data, label):
        """One optimizer step on a batch; returns (prediction, {loss name: loss})."""
        self.optimizer.zero_grad()
        pred = self.model(data)
        loss, loss_logs = self.model.loss_func(pred, label)
        loss.backward()
        self.optimizer.step()
        return pred, loss_logs

    def _begin(self, dataset):
        self._items = len(dataset)
        self._began = time.time()

    def train(self, dataset, log_interval=100):
        """One pass over `dataset`; every `log_interval` steps the losses are logged and the model is checkpointed."""
        self._begin(dataset)
        self.model.train()
        for step, (data, label) in enumerate(dataset):
            pred, loss_logs = self.update(data, label)
            if step % log_interval:
                continue
            self.log('Train', step, loss_logs, data, label, pred)
            self.log_figure(step, loss_logs, data, label, pred)
            self.save()

    def play(self, dataset, log=True, log_figure=False):
        """Loads the checkpoint in `logdir` (which leaves the model in eval mode) and scores it on `dataset`."""
        self._begin(dataset)
        self.load()
        with torch.no_grad():
            for step, (data, label) in enumerate(dataset):
                pred = self.model(data)
                loss_logs = self.model.loss_func(pred, label)[1]
                if log:
                    self.log('Eval', step, loss_logs, data, label, pred)
                if log_figure:
                    self.log_figure(step, loss_logs, data, label, pred)

    def log(self, run_mode, step, loss_logs, data, label, pred, width=42):
        """Prints the losses of `step` with the time spent and left, and writes them as scalars `<run_mode>/<name>`."""
        now = time.time()
        spent = now - self._began
        left = spent * (self._items - step - 1) / (step + 1)
        report = [f" step {step} of {self._items} ".center(width, "-")]
        for name, value in loss_logs.items():
            value = float(value.detach()) if torch.is_tensor(value) else float(value)
            report.append(f"{run_mode + '/' + name:>{width // 2}} = {value:.6g}")
            if self.logger is not None:
                self.logger.add_scalar(f"{run_mode}/{name}", value, global_step=step, walltime=now)
        if self.logger is not None:
            self.logger.flush()
        report.append(f"{'spent':>{width // 2}} = {spent:.1f} s, about {max(left, 0.0):.1f} s to go")
        print("\n".join(report))

    def save(self):
        os.makedirs(self.logdir, exist_ok=True)
        self.model.save(self.logdir)

    def load(self):
        self.model.load(self.logdir)

    def log_figure(self, step, loss_logs, data, label, predicted):
        """Hook for subclasses that draw; nothing is drawn here."""

    def destroy(self):
        if self.logger is not None:
            self.logger.close()
        self.model = self.optimizer = None
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


def run_module(run_mode, model, dataset, model_name, train_log_interval=100, play_log=True, play_log_figure=False,
               log_root="./logs", runner_class=ModuleRunner, lr=1e-4, weight_decay=1e-05, device='cuda:0'):
    """`train` starts a new run `<log_root>/<time stamp>_<model_name>` and checkpoints into it.  `play` loads the newest such
    run and writes its scalars to a new run under `<log_root>_play/<model_name>/`."""
    if run_mode not in ("train", "play"):
        raise NotImplementedError(f"run_module: run_mode {run_mode!r} (train or play)")
    print(f"run_module: {run_mode} {model_name}")
    if run_mode == "train":
        checkpoints = scalars = datetime_logdir(log_root, model_name)
        settings = dict(lr=lr, weight_decay=weight_decay)
    else:
        checkpoints = latest_logdir(log_root, model_name)
        scalars = datetime_logdir(f"{log_root}_play/{model_name}", model_name)
        settings = {}
    runner = runner_class(model, logdir=checkpoints, tensorboard_logdir=scalars, device=device, **settings)
    try:
        if run_mode == "train":
            runner.train(dataset, train_log_interval)
        else:
            runner.play(dataset, log=play_log, log_figure=play_log_figure)
    finally:
        runner.destroy()
