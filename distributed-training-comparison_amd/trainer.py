"""Trainer and CLI mirroring the reference's src/single and src/ddp entry points.

Same flags (src/ddp/config.py:4-39; src/single/config.py differs only in ckpt-path/epoch
defaults), same flow (main.py -> Trainer.fit -> _train_epoch -> validate -> checkpoint -> test),
same step (single/trainer.py:131-147, ddp/trainer.py:149-167 incl. the per-step dist.barrier()),
on the native modules. Differences, all forced by this environment and documented in DESIGN.md:
CIFAR-100 is replaced by a seeded synthetic stand-in (no download), TensorBoard scalars go to
``scalars.jsonl`` (tensorboardX is not installed), and the model always computes in bf16.
"""
from __future__ import annotations

import argparse
import glob
import json
import logging
import os
import re
import time
from typing import Tuple

import torch
import torch.distributed as dist

from . import checkpoint
from . import data as D
from .amp import GradScaler, autocast
from .ema import ModelEma
from .nn import CrossEntropyLoss, ResNet18, SyncBatchNorm
from .optim import LARS, SAM, SGD, Adam, AdamW, clip_grad_norm_
from .parallel import DDP, DataParallel, PowerSGDState, barrier, bf16_compress_hook, powerSGD_hook


def load_config(argv=None, mode: str = "ddp"):
    p = argparse.ArgumentParser()
    p.add_argument("--dset", type=str, default="cifar100")
    p.add_argument("--dpath", type=str, default="data/")
    p.add_argument("--ckpt-path", type=str, default=f"src/{mode}/checkpoints/")
    p.add_argument("--seed", type=int, default=42, help="Seed for reproducibility")
    p.add_argument("--workers", type=int, default=4)
    p.add_argument("--eval-step", type=int, default=300)
    p.add_argument("--amp", action="store_true", default=False, help="PyTorch(>=1.6.x) AMP")
    p.add_argument("--contain-test", action="store_true", default=False)
    if mode == "ddp":
        p.add_argument("--world-size", type=int, default=1, help="Total number of processes to run")
        p.add_argument("--rank", type=int, default=0)
        p.add_argument("--dist-backend", type=str, default="nccl")
        p.add_argument("--dist-url", default="tcp://127.0.0.1:3456", type=str)
        p.add_argument("--sync-bn", action="store_true", default=False,
                       help="SyncBatchNorm.convert_sync_batchnorm (README.md:40; off in the reference)")
        # not in the reference: torch's ddp.register_comm_hook(None, default_hooks.bf16_compress_hook)
        p.add_argument("--grad-compress", choices=("none", "bf16", "powersgd"), default="none",
                       help="bf16: all-reduce the gradient buckets in bf16 (half the bytes per step); the optimizer "
                            "still reads fp32 gradients. powersgd: rank-r PowerSGD with error feedback (torch's "
                            "powerSGD_hook): two all-reduces of tens of kilobytes per step after the start iteration")
        p.add_argument("--powersgd-rank", type=int, default=2, choices=(1, 2, 3, 4),
                       help="--grad-compress powersgd: matrix_approximation_rank")
        p.add_argument("--powersgd-start-iter", type=int, default=1000,
                       help="--grad-compress powersgd: start_powerSGD_iter, the plain all-reduced steps before the "
                            "compression starts (at least 2)")
    p.add_argument("--epoch", type=int, default=200 if mode == "single" else 100)
    p.add_argument("--batch-size", type=int, default=128)
    p.add_argument("--model", type=str, default="resnet18")
    p.add_argument("--lr", type=float, default=0.1)
    p.add_argument("--weight-decay", type=float, default=0.0001)
    p.add_argument("--lr-decay-step-size", type=int, default=60)
    p.add_argument("--lr-decay-gamma", type=float, default=0.1)
    # not in the reference, whose README suggests the experiment ("e.g. using ADAM optimizer")
    p.add_argument("--optimizer", type=str, default="sgd", choices=("sgd", "adam", "adamw", "lars"),
                   help="fused flat-buffer optimizer; --lr and --weight-decay pass through (lars: the sgd branch's "
                        "momentum 0.9 + Nesterov with a per-tensor trust ratio, for large global batches)")
    p.add_argument("--lars-trust-coef", type=float, default=1e-3,
                   help="--optimizer lars: ratio = coef * ||p|| / (||g|| + weight_decay * ||p|| + eps)")
    p.add_argument("--lars-clip", action="store_true", default=False,
                   help="--optimizer lars: LARC clipping, ratio = min(ratio / lr, 1)")
    p.add_argument("--warmup-epochs", type=int, default=0,
                   help="linear warm-up: epoch e < N runs at lr * (e + 1) / N and StepLR's count starts at epoch N "
                        "(0 = off: the reference's plain StepLR)")
    p.add_argument("--clip-grad-norm", type=float, default=0.0,
                   help="clip the global gradient L2 norm to this value before each step (0 = off)")
    # not in the reference either: the regularizers people change first at larger global batches
    p.add_argument("--label-smoothing", type=float, default=0.0,
                   help="CrossEntropyLoss(label_smoothing=) of the TRAINING loss; validate() and test() report "
                        "the plain cross-entropy whatever this is (also with --fused-eval)")
    p.add_argument("--mixup-alpha", type=float, default=0.0,
                   help="Mixup with lam ~ Beta(alpha, alpha) per batch, on the device (needs --device-data; 0 = off)")
    p.add_argument("--cutmix-alpha", type=float, default=0.0,
                   help="CutMix with lam ~ Beta(alpha, alpha) per batch, on the device (needs --device-data; 0 = off)")
    p.add_argument("--mix-prob", type=float, default=1.0,
                   help="probability that a batch is mixed; with both alphas set each kind is picked half the time")
    # the data side of the same recipes (timm --aa rand-m9-n2 --reprob 0.25, torchvision --auto-augment ta_wide)
    p.add_argument("--auto-augment", choices=["none", "randaugment", "trivialwide"], default="none",
                   help="augmentation policy applied per sample on the device, between the flip and Normalize "
                        "(needs --device-data)")
    p.add_argument("--ra-num-ops", type=int, default=2, help="--auto-augment randaugment: ops per sample, 1..4")
    p.add_argument("--ra-magnitude", type=int, default=9,
                   help="--auto-augment randaugment: magnitude bin of 31, 0..30")
    p.add_argument("--random-erasing", type=float, default=0.0,
                   help="RandomErasing probability per sample, value 0, on the device (needs --device-data; not with "
                        "--mixup-alpha / --cutmix-alpha; 0 = off)")
    # timm's / torchvision's --model-ema: the weights worth keeping at large batches and under Mixup / CutMix
    p.add_argument("--model-ema", action="store_true", default=False,
                   help="keep an exponential moving average of the weights and running statistics on the device "
                        "(ema.ModelEma); validate() reports it, the best checkpoint stores it")
    p.add_argument("--model-ema-decay", type=float, default=0.9998, help="--model-ema: decay, in [0, 1)")
    p.add_argument("--model-ema-warmup", action="store_true", default=False,
                   help="--model-ema: decay_t = min(decay, (1 + t) / (10 + t)) over the updates t")
    p.add_argument("--model-ema-steps", type=int, default=1, help="--model-ema: update on every N-th global step")
    # not in the reference: the global batch of the large-batch recipes above on few GPUs
    p.add_argument("--accum-steps", type=int, default=1,
                   help="gradient accumulation: one optimizer step per N loader iterations, on the mean gradient of "
                        "their N micro-batches (ddp: one all-reduce per N backwards, DDP.no_sync()). The last "
                        "iteration of an epoch closes a shorter window, still divided by N (single and ddp only)")
    # not in the reference: sharpness-aware minimisation (Foret et al. 2021) around whichever --optimizer
    p.add_argument("--sam-rho", type=float, default=0.0,
                   help="SAM: every optimizer step takes its gradient at the worst point of the rho-ball around the "
                        "weights, found along this rank's own gradient (two forward / backward passes per step; "
                        "0 = off; typical 0.05; single and ddp only, not with --accum-steps > 1)")
    p.add_argument("--sam-adaptive", action="store_true", default=False,
                   help="--sam-rho: ASAM (Kwon et al. 2021), the ball scaled per weight by |w|; typical rho 0.5 to 2.0")
    # synthetic-data size knobs (not in the reference: CIFAR-100 cannot be downloaded here)
    p.add_argument("--synthetic-train", type=int, default=50000)
    p.add_argument("--synthetic-test", type=int, default=10000)
    p.add_argument("--max-steps", type=int, default=0, help="stop each epoch after N steps (0 = full epoch)")
    p.add_argument("--device-data", action="store_true", default=False,
                   help="HBM-resident uint8 dataset + on-GPU crop/flip/normalize (data.DeviceLoader)")
    p.add_argument("--fused-eval", action="store_true", default=False,
                   help="validate()/test() on the device: one native call per batch (eval forward + loss + top-k "
                        "counts), one device-to-host copy per evaluation (ResNet.evaluate); same numbers")
    # not in the reference, which saves the best epoch's weights and cannot continue a run
    p.add_argument("--checkpoint-every", type=int, default=0,
                   help="write the full training state to <version dir>/last.ckpt after every N-th epoch and after "
                        "the last one (0 = off; single and ddp only)")
    p.add_argument("--resume", type=str, default=None, metavar="PATH",
                   help="continue the run of a version directory (or its last.ckpt) in that directory, bit for bit "
                        "as if it had not stopped; the flags that shape the state must be the saved run's, --epoch "
                        "may be raised (single and ddp only)")
    if mode == "dp":  # not in the reference (nn.DataParallel takes every visible GPU): replica placement
        p.add_argument("--device-ids", type=lambda v: [int(d) for d in v.split(",")], default=None,
                       help="comma-separated GPU ids of the replicas (may repeat); default: all visible")
    h = p.parse_args(argv)
    if not 0.0 <= h.label_smoothing <= 1.0:
        p.error("--label-smoothing must be in [0, 1]")
    if h.mixup_alpha < 0 or h.cutmix_alpha < 0 or not 0.0 <= h.mix_prob <= 1.0:
        p.error("--mixup-alpha / --cutmix-alpha must be >= 0 and --mix-prob in [0, 1]")
    if mode == "ddp" and h.powersgd_start_iter < 2:
        p.error("--powersgd-start-iter must be at least 2")
    if h.warmup_epochs < 0 or not h.lars_trust_coef > 0:
        p.error("--warmup-epochs must be >= 0 and --lars-trust-coef > 0")
    if (h.mixup_alpha > 0 or h.cutmix_alpha > 0) and not h.device_data:
        p.error("--mixup-alpha / --cutmix-alpha need --device-data (the host loader does not mix)")
    if not 1 <= h.ra_num_ops <= 4 or not 0 <= h.ra_magnitude <= 30 or not 0.0 <= h.random_erasing <= 1.0:
        p.error("--ra-num-ops must be in [1, 4], --ra-magnitude in [0, 30] and --random-erasing in [0, 1]")
    if (h.auto_augment != "none" or h.random_erasing > 0) and not h.device_data:
        p.error("--auto-augment / --random-erasing need --device-data (the host loader applies no policy)")
    if h.random_erasing > 0 and (h.mixup_alpha > 0 or h.cutmix_alpha > 0):
        p.error("--random-erasing does not combine with --mixup-alpha / --cutmix-alpha")
    if not 0.0 <= h.model_ema_decay < 1.0 or h.model_ema_steps < 1:
        p.error("--model-ema-decay must be in [0, 1) and --model-ema-steps >= 1")
    if h.accum_steps < 1:
        p.error("--accum-steps must be >= 1")
    if mode == "dp" and h.accum_steps > 1:
        p.error("--accum-steps > 1 is not available under DataParallel (single and ddp only)")
    if not h.sam_rho >= 0.0:
        p.error("--sam-rho must be >= 0")
    if h.sam_rho > 0 and h.accum_steps > 1:
        p.error("--sam-rho is not available with --accum-steps > 1 (its first backward is a whole step's gradient)")
    if h.sam_rho > 0 and mode == "dp":
        p.error("--sam-rho is not available under DataParallel (single and ddp only)")
    if h.checkpoint_every < 0:
        p.error("--checkpoint-every must be >= 0")
    if mode == "dp" and (h.checkpoint_every > 0 or h.resume is not None):
        p.error("--checkpoint-every / --resume are not available under DataParallel (single and ddp only)")
    return h


# The flags a resumed run must share with the run that wrote the checkpoint: they shape the saved state (which
# optimizer, scaler, EMA, hook state exist and what they mean) or the data stream of the epochs still to come.
# --epoch, --eval-step, --contain-test, --workers, --checkpoint-every, --max-steps, --fused-eval, the paths and the
# process-group address may differ.
RESUME_KEYS = (
    "dset", "model", "seed", "batch_size", "synthetic_train", "device_data", "amp",
    "optimizer", "lr", "weight_decay", "lars_trust_coef", "lars_clip", "clip_grad_norm",
    "lr_decay_step_size", "lr_decay_gamma", "warmup_epochs",
    "label_smoothing", "mixup_alpha", "cutmix_alpha", "mix_prob",
    "auto_augment", "ra_num_ops", "ra_magnitude", "random_erasing",
    "model_ema", "model_ema_decay", "model_ema_warmup", "model_ema_steps",
    "accum_steps", "sam_rho", "sam_adaptive",
    "world_size", "sync_bn", "grad_compress", "powersgd_rank", "powersgd_start_iter",
)


def hparam_mismatch(saved: dict, current: dict) -> list:
    """[(key, saved value, current value)] over RESUME_KEYS, in their order; a key neither side has (a flag of
    another mode) is equal."""
    missing = object()
    out = []
    for k in RESUME_KEYS:
        a, b = saved.get(k, missing), current.get(k, missing)
        if a is missing and b is missing:
            continue
        if a is missing or b is missing or a != b:
            out.append((k, None if a is missing else a, None if b is missing else b))
    return out


def resolve_resume(path: str) -> Tuple[str, str]:
    """(version directory, checkpoint file) of --resume PATH, a version directory or its last.ckpt."""
    file = os.path.join(path, "last.ckpt") if os.path.isdir(path) else path
    if not os.path.isfile(file):
        raise checkpoint.CheckpointError(f"--resume {path}: there is no last.ckpt (was the run started with "
                                         "--checkpoint-every?)")
    return os.path.dirname(os.path.abspath(file)), file


def accuracy(output, target, topk=(1,)):
    """utils.py:18-31."""
    maxk = max(topk)
    batch_size = target.size(0)
    _, pred = output.topk(maxk, 1, True, True)
    pred = pred.t()
    correct = pred.eq(target.reshape(1, -1).expand_as(pred))
    return [correct[:k].reshape(-1).float().sum(0).mul_(100.0 / batch_size) for k in topk]


class AverageMeter:
    """utils.py:34-48."""

    def __init__(self):
        self.val = self.avg = self.sum = 0.0
        self.count = 0

    def update(self, val: float, n: int = 1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def make_criteria(hparams):
    """(training criterion, evaluation criterion): --label-smoothing shapes the training loss only; validate()
    and test() keep the plain cross-entropy (the number --fused-eval's device metrics report too). With the
    default 0 both are the one CrossEntropyLoss() the reference builds (trainer.py:40)."""
    eps = float(getattr(hparams, "label_smoothing", 0.0))
    plain = CrossEntropyLoss()
    return (CrossEntropyLoss(label_smoothing=eps) if eps > 0 else plain), plain


def mix_kwargs(hparams) -> dict:
    """The train DeviceLoader's Mixup / CutMix keywords (none with the default flags). Mixing is per process:
    per rank under DDP, before the scatter under DataParallel (the loss sees the gathered logits)."""
    ma, ca = float(getattr(hparams, "mixup_alpha", 0.0)), float(getattr(hparams, "cutmix_alpha", 0.0))
    if ma <= 0 and ca <= 0:
        return {}
    return {"mixup_alpha": ma, "cutmix_alpha": ca, "mix_prob": float(getattr(hparams, "mix_prob", 1.0))}


def policy_kwargs(hparams) -> dict:
    """The train DeviceLoader's augmentation-policy and RandomErasing keywords (none with the default flags)."""
    policy, erase = getattr(hparams, "auto_augment", "none"), float(getattr(hparams, "random_erasing", 0.0))
    if policy == "none" and erase <= 0:
        return {}
    return {"policy": policy, "policy_num_ops": int(getattr(hparams, "ra_num_ops", 2)),
            "policy_magnitude": int(getattr(hparams, "ra_magnitude", 9)), "erase_prob": erase}


def make_scheduler(optimizer, hparams):
    """The per-epoch learning-rate schedule. Without --warmup-epochs: the reference's StepLR (trainer.py:101-105),
    the same object as ever. With N warm-up epochs: epoch e < N runs at lr * (e + 1) / N, and from epoch N on
    StepLR's rule counted from there, lr * gamma ** ((e - N) // step_size). Host-only: every optimizer passes its
    lr to the kernel per launch."""
    n, step, gamma = int(getattr(hparams, "warmup_epochs", 0)), hparams.lr_decay_step_size, hparams.lr_decay_gamma
    if n <= 0:
        return torch.optim.lr_scheduler.StepLR(optimizer, step_size=step, gamma=gamma)
    return torch.optim.lr_scheduler.LambdaLR(
        optimizer, lambda e: (e + 1) / n if e < n else gamma ** ((e - n) // step))


class Trainer:
    def __init__(self, hparams, model, scaler, rank: int = 0, ngpus_per_node: int = 1, distributed: bool = False,
                 data_parallel: bool = False):
        self.hparams = hparams
        self.rank = rank
        self.distributed = distributed
        self.data_parallel = data_parallel
        self.checkpoint_every = int(getattr(hparams, "checkpoint_every", 0) or 0)
        self.start_epoch = 0
        resume = None
        if getattr(hparams, "resume", None):  # read on every rank, before anything is built
            resume_dir, resume_file = resolve_resume(hparams.resume)
            resume = checkpoint.load(resume_file)
        self.device = torch.device("cuda", rank if distributed else torch.cuda.current_device())
        self.model = model.to(self.device)
        if data_parallel:
            self.model = DataParallel(self.model, device_ids=getattr(hparams, "device_ids", None))  # dp/trainer.py:27
        if distributed:
            self.model = DDP(self.model, device_ids=[rank], find_unused_parameters=True)   # ddp/trainer.py:31
            if getattr(hparams, "grad_compress", "none") == "bf16":
                self.model.register_comm_hook(None, bf16_compress_hook)
            elif getattr(hparams, "grad_compress", "none") == "powersgd":
                self.model.register_comm_hook(PowerSGDState(matrix_approximation_rank=hparams.powersgd_rank,
                                                            start_powerSGD_iter=hparams.powersgd_start_iter),
                                              powerSGD_hook)
            hparams.batch_size = int(hparams.batch_size / ngpus_per_node)                  # ddp/trainer.py:34
        if resume is not None:
            diff = hparam_mismatch(resume["extra"]["hparams"], vars(hparams))
            if diff:
                raise checkpoint.CheckpointError(
                    f"--resume {hparams.resume}: the checkpoint was written under other flags: "
                    + "; ".join(f"{k}: saved {a!r}, now {b!r}" for k, a, b in diff))
        self.scaler = scaler
        self.optimizer, self.lr_scheduler = self.configure_optimizers()
        self.criterion, self.eval_criterion = make_criteria(hparams)
        # --model-ema: every DDP rank keeps its own (identical) EMA; under DataParallel it follows the master
        # module on device_ids[0]. Built behind the wrappers, so it starts from the broadcast weights.
        self.ema = None
        self.val_raw_acc = None
        if getattr(hparams, "model_ema", False):
            self.ema = ModelEma(self.model, decay=hparams.model_ema_decay, warmup=hparams.model_ema_warmup)
        if getattr(hparams, "device_data", False):
            self._device_loaders(hparams, distributed)
        else:
            ds = D.SyntheticCIFAR100(n=hparams.synthetic_train)
            self.train_loader, self.train_sampler, self.val_loader = D.get_trn_val_loader(
                batch_size=hparams.batch_size, valid_size=0.1, num_workers=hparams.workers, pin_memory=True,
                distributed=distributed, dataset=ds)
            self.test_loader = D.get_tst_loader(batch_size=hparams.batch_size, num_workers=1, pin_memory=True,
                                                distributed=distributed, n=hparams.synthetic_test)
        self.global_step = 0
        # optimizer steps taken (--accum-steps N: one per window of N loader iterations; N = 1: == global_step)
        self.optimizer_step = 0
        self.accum_steps = int(getattr(hparams, "accum_steps", 1))
        self.sam = isinstance(self.optimizer, SAM)
        if self.accum_steps > 1:
            self._module_for_eval().grad_accum_steps = self.accum_steps
        self.global_top1_acc = 0.0
        self.eval_step = hparams.eval_step
        self.version = None
        if resume is not None:  # the run goes on in its own directory (every rank knows it)
            self.save_path = resume_dir
        if rank == 0:
            if resume is not None:
                m = re.fullmatch(r"version-(\d+)", os.path.basename(resume_dir))
                self.version = int(m.group(1)) if m else None
            else:
                self.version = 0
                while True:
                    self.save_path = os.path.join(hparams.ckpt_path, f"version-{self.version}")
                    if not os.path.exists(self.save_path):
                        os.makedirs(self.save_path)
                        break
                    self.version += 1
            logging.basicConfig(filename=os.path.join(self.save_path, "experiment.log"), level=logging.INFO,
                                format="%(asctime)s > %(message)s", force=True)
            if resume is None:  # a resumed run leaves hparams.json as it is
                with open(os.path.join(self.save_path, "hparams.json"), "w") as f:
                    json.dump(vars(hparams), f, indent=1)
            self._scalars = open(os.path.join(self.save_path, "scalars.jsonl"), "a")
        # every rank of a checkpointing ddp run writes a file of its own next to rank 0's (_write_checkpoint)
        self.global_rank = dist.get_rank() if distributed else 0
        self._rank_files = distributed and (dist.get_world_size() > 1
                                            or getattr(hparams, "grad_compress", "none") == "powersgd")
        if resume is None and self._rank_files and self.checkpoint_every > 0 and dist.get_world_size() > 1:
            box = [self.save_path if rank == 0 else None]  # rank 0's new directory, for the others' files
            dist.broadcast_object_list(box, src=0)
            self.save_path = box[0]
        if resume is not None:
            self._restore(resume)

    def _rank_file(self) -> str:
        return os.path.join(self.save_path, f"last.rank{self.global_rank}.ckpt")

    def _restore(self, state) -> None:
        """--resume: `state` (last.ckpt, read by every rank) into the freshly built objects, this rank's own file
        (the PowerSGD hook state with its error-feedback buffer, and this rank's generators) on top; the random
        generators last, since building the model and the loaders has drawn from them."""
        mine = None
        if self._rank_files:
            if not os.path.isfile(self._rank_file()):
                raise checkpoint.CheckpointError(f"--resume: {self._rank_file()} is missing (every rank of a ddp "
                                                 "run writes one next to last.ckpt)")
            mine = checkpoint.load(self._rank_file())
            if mine["epoch"] != state["extra"]["epoch"]:
                raise checkpoint.CheckpointError(f"--resume: {self._rank_file()} is of epoch {mine['epoch']}, "
                                                 f"last.ckpt of epoch {state['extra']['epoch']}")
            self.model.load_comm_hook_state_dict(mine["hook"])
        extra = checkpoint.restore(state, self.model, self.optimizer, self.scaler, self.ema, self.lr_scheduler)
        self.start_epoch = int(extra["epoch"])
        self.global_step, self.optimizer_step = int(extra["global_step"]), int(extra["optimizer_step"])
        self.global_top1_acc = float(extra["global_top1_acc"])
        if mine is not None:
            checkpoint.set_rng_state(mine["rng"])
        logging.info(f"Resumed from {self.save_path}: next epoch {self.start_epoch}, global step {self.global_step}")

    def _write_checkpoint(self, epoch: int) -> None:
        """--checkpoint-every N: after epoch `epoch` (the scheduler has stepped) rank 0 writes last.ckpt -- the
        whole training state plus the next epoch, the step counts, the best accuracy so far with its file's name
        and the flags --, every rank of a ddp run its last.rank<r>.ckpt first. An epoch boundary is the only point
        where no gradient-accumulation window, SAM perturbation or pending clip is open."""
        n = self.checkpoint_every
        if n <= 0 or not ((epoch + 1) % n == 0 or epoch == self.hparams.epoch - 1):
            return
        t0 = time.perf_counter()
        if self._rank_files:
            checkpoint.save(self._rank_file(), {
                checkpoint.FORMAT_KEY: checkpoint.FORMAT, "rank": self.global_rank, "epoch": epoch + 1,
                "hook": checkpoint.to_plain(self.model.comm_hook_state_dict(), "hook"),
                "rng": checkpoint.get_rng_state()})
        if self.rank != 0:
            return
        best = glob.glob(os.path.join(self.save_path, "best_model_*.pt"))
        extra = {"epoch": epoch + 1, "global_step": self.global_step, "optimizer_step": self.optimizer_step,
                 "global_top1_acc": float(self.global_top1_acc),
                 "best_model": os.path.basename(best[0]) if best else None, "hparams": vars(self.hparams)}
        path = os.path.join(self.save_path, "last.ckpt")
        checkpoint.save(path, checkpoint.capture(self.model, self.optimizer, self.scaler, self.ema,
                                                 self.lr_scheduler, extra))
        logging.info(f"Checkpoint after epoch {epoch}: {os.path.getsize(path) / 2 ** 20:.1f} MiB in "
                     f"{time.perf_counter() - t0:.2f} s")

    def _device_loaders(self, hparams, distributed):
        """--device-data: the loaders of dataset.py:15-168 with the transforms on the GPU
        (D.DeviceLoader over HBM-resident uint8 CIFAR-shaped data): same 45k/5k split, the same
        DistributedSampler (DDP) or per-epoch random order (single/dp), drop_last on train, train
        transform with crop+flip, valid without, test normalized with the ImageNet statistics of
        dataset.py:139-142 and sharded by a DistributedSampler under DDP (dataset.py:158)."""
        imgs, tg = D.synthetic_cifar_u8(n=hparams.synthetic_train, seed=hparams.seed)
        train_idx, valid_idx = D.train_valid_split(len(tg), 0.1, True)
        sampler = (D.DistributedSampler(train_idx) if distributed
                   else torch.utils.data.SubsetRandomSampler(list(range(len(train_idx)))))
        bs = hparams.batch_size
        self.train_loader = D.DeviceLoader(imgs, tg, bs, subset_idx=train_idx, sampler=sampler, train=True,
                                           seed=hparams.seed, device=self.device, **mix_kwargs(hparams),
                                           **policy_kwargs(hparams))
        self.train_sampler = self.train_loader
        self.val_loader = D.DeviceLoader(imgs, tg, bs, subset_idx=valid_idx, train=False, drop_last=False,
                                         device=self.device)
        timgs, ttg = D.synthetic_cifar_u8(n=hparams.synthetic_test, seed=hparams.seed + 1)
        # DistributedSampler(test_dataset) with its default shuffle=True, exactly dataset.py:158: rank 0
        # tests the same (shuffled) 1/W subset the reference's rank 0 does
        tsampler = D.DistributedSampler(range(len(ttg))) if distributed else None
        self.test_loader = D.DeviceLoader(timgs, ttg, bs, sampler=tsampler, train=False, drop_last=False,
                                          mean=D.IMAGENET_MEAN, std=D.IMAGENET_STD, device=self.device)

    def _log_scalar(self, tag, values, step):
        if self.rank == 0:
            self._scalars.write(json.dumps({"tag": tag, "step": step, **values}) + "\n")
            self._scalars.flush()

    def configure_optimizers(self):
        h = self.hparams
        if h.optimizer == "sgd":
            optimizer = SGD(self.model.parameters(), lr=h.lr, weight_decay=h.weight_decay,
                            momentum=0.9, nesterov=True)                                  # trainer.py:92-98
        elif h.optimizer == "lars":  # the sgd branch plus the trust ratio
            optimizer = LARS(self.model.parameters(), lr=h.lr, weight_decay=h.weight_decay, momentum=0.9,
                             nesterov=True, trust_coef=h.lars_trust_coef, trust_clip=h.lars_clip)
        else:
            cls = {"adam": Adam, "adamw": AdamW}[h.optimizer]
            optimizer = cls(self.model.parameters(), lr=h.lr, weight_decay=h.weight_decay)
        if getattr(h, "sam_rho", 0.0) > 0:  # shares param_groups with the base: the schedule drives the base's lr
            optimizer = SAM(optimizer, rho=h.sam_rho, adaptive=getattr(h, "sam_adaptive", False))
        return optimizer, make_scheduler(optimizer, h)

    def save_checkpoint(self, epoch: int, val_acc: float, model) -> None:
        logging.info(f"Val acc increased ({self.global_top1_acc:.4f} -> {val_acc:.4f}). Saving model ...")
        new_path = os.path.join(self.save_path, f"best_model_epoch_{epoch}_acc_{val_acc:.4f}.pt")
        for filename in glob.glob(os.path.join(self.save_path, "*.pt")):
            os.remove(filename)
        state = model.state_dict()
        if self.ema is not None:  # the averaged weights under the model's own keys: test() loads them as ever
            ema_state = self.ema.state_dict()
            prefix = "module." if (self.distributed or self.data_parallel) else ""
            state = {k: ema_state[k[len(prefix):]] for k in state}
        torch.save({k: v.contiguous() for k, v in state.items()}, new_path)
        self.global_top1_acc = val_acc

    def fit(self):
        for epoch in range(self.start_epoch, self.hparams.epoch):
            if self.distributed or isinstance(self.train_loader, D.DeviceLoader):
                self.train_sampler.set_epoch(epoch)                                       # trainer.py:125
            logging.info(f"* Learning Rate: {self.optimizer.param_groups[0]['lr']:.5f}")
            result = self._train_epoch(epoch)
            if self.rank == 0 and result["val_acc"] > self.global_top1_acc:
                self.save_checkpoint(epoch, result["val_acc"], self.model)
            self.lr_scheduler.step()
            self._write_checkpoint(epoch)
        return self.version

    def _backward(self, loss, closing: bool) -> None:
        """loss.backward(); inside a --accum-steps window (not `closing`) under the model's accumulate() /
        DDP's no_sync(): the gradients are added to the window's sum and nothing is all-reduced."""
        if closing:
            loss.backward()
        else:
            with (self.model.no_sync() if self.distributed else self.model.accumulate()):
                loss.backward()

    def _loss(self, img, label):
        if self.hparams.amp:
            with autocast():
                return self.criterion(self.model(img), label)
        return self.criterion(self.model(img), label)

    def _sam_step(self, img, label):
        """One optimizer step with --sam-rho: the loss at w (returned: the one that is logged) and its backward
        inside local_grads() -- this rank's own gradient, nothing all-reduced --, first_step() to w + e, then the
        same (already mixed) batch and target again: loss at w + e, the per-step barrier (still one per optimizer
        step), the all-reduced backward and the unscale_ / clip / step / EMA / update sequence of the plain step.
        The optimizer's step() first restores w and the BatchNorm running state of the first forward."""
        amp, scaler = self.hparams.amp, self.scaler
        loss = self._loss(img, label)
        with self._module_for_eval().local_grads():
            (scaler.scale(loss) if amp else loss).backward()
        self.optimizer.first_step(scaler if amp else None)
        loss2 = self._loss(img, label)
        if self.distributed:
            barrier()
        (scaler.scale(loss2) if amp else loss2).backward()
        if amp:
            if self.hparams.clip_grad_norm > 0:
                scaler.unscale_(self.optimizer)
                clip_grad_norm_(self.model.parameters(), self.hparams.clip_grad_norm, scaler=scaler)
            scaler.step(self.optimizer)
            self._ema_update(scaler.found_inf)
            scaler.update()
        else:
            if self.hparams.clip_grad_norm > 0:
                clip_grad_norm_(self.model.parameters(), self.hparams.clip_grad_norm)
            self.optimizer.step()
            self._ema_update(None)
        return loss

    def _train_epoch(self, epoch: int) -> dict:
        """One epoch of the reference's step. --accum-steps N > 1: backwards 1..N-1 of a window of N loader
        iterations accumulate; the N-th closes the window and is followed by the unscale_ / clip / step / EMA /
        scaler.update sequence, which therefore runs -- and counts -- once per optimizer step. The epoch's last
        iteration (also an early end through --max-steps) closes a shorter window; its gradient is still the sum
        divided by N (PyTorch Lightning's accumulate_grad_batches does the same). Logging, --eval-step and the
        per-iteration barrier keep counting loader iterations."""
        train_loss = AverageMeter()
        self.model.train()
        n_acc = self.accum_steps
        n_iter = len(self.train_loader) if n_acc > 1 else 0  # (read only to find a window's early end)
        if n_acc > 1 and self.hparams.max_steps:
            n_iter = min(n_iter, self.hparams.max_steps)
        for step, (img, label) in enumerate(self.train_loader):
            if self.hparams.max_steps and step >= self.hparams.max_steps:
                break
            closing = n_acc == 1 or (step + 1) % n_acc == 0 or step + 1 == n_iter
            img = img.to(self.device, non_blocking=True)
            label = label.to(self.device, non_blocking=True)
            self.optimizer.zero_grad()
            if self.sam:
                loss = self._sam_step(img, label)
            elif self.hparams.amp:
                with autocast():
                    logit = self.model(img)
                    loss = self.criterion(logit, label)
                if self.distributed:
                    barrier()  # dist.barrier() on the native communicator            # trainer.py:156
                self._backward(self.scaler.scale(loss), closing)
                if closing:
                    if self.hparams.clip_grad_norm > 0:  # torch's documented order: unscale_, clip, step
                        self.scaler.unscale_(self.optimizer)
                        clip_grad_norm_(self.model.parameters(), self.hparams.clip_grad_norm, scaler=self.scaler)
                    self.scaler.step(self.optimizer)
                    self._ema_update(self.scaler.found_inf)  # before update(), which clears found_inf
                    self.scaler.update()
            else:
                logit = self.model(img)
                loss = self.criterion(logit, label)
                if self.distributed:
                    barrier()                                                             # trainer.py:163
                self._backward(loss, closing)
                if closing:
                    if self.hparams.clip_grad_norm > 0:
                        clip_grad_norm_(self.model.parameters(), self.hparams.clip_grad_norm)
                    self.optimizer.step()
                    self._ema_update(None)
            train_loss.update(loss.item())
            self.global_step += 1
            if closing:
                self.optimizer_step += 1
            if self.rank == 0 and self.global_step % self.eval_step == 0:
                tag = "DDP" if self.distributed else ("DP" if self.data_parallel else "Single")
                logging.info(f"[{tag} Version {self.version} Epoch {epoch}] "
                             f"global step: {self.global_step}, train loss: {loss.item():.3f}")
        result = {"val_loss": 0.0, "val_acc": 0.0, "train_loss": train_loss.avg}
        if self.rank == 0:
            val_loss, val_acc = self.validate(epoch)
            self._log_scalar("lr", {"lr": self.optimizer.param_groups[0]["lr"]}, epoch)
            self._log_scalar("loss/epoch", {"val": val_loss, "train": train_loss.avg}, epoch)
            acc = {"val": val_acc}
            if self.ema is not None:
                acc["val_raw"] = self.val_raw_acc
            self._log_scalar("acc/epoch", acc, epoch)
            logging.info(f"** global step: {self.global_step}, val loss: {val_loss:.3f}, val_acc: {val_acc:.2f}%")
            result.update(val_loss=val_loss, val_acc=val_acc)
        return result

    def _module(self):
        # DDP: rank 0 evaluates the unwrapped module; DP evaluates through the replicas
        # (dp/trainer.py:121-129 calls self.model, the DataParallel wrapper)
        return self.model.module if self.distributed else self.model

    def _module_for_eval(self):
        """--fused-eval: the native ResNet that ``evaluate`` runs on. DDP: rank 0's unwrapped module, as
        the default path. DP: the wrapped module on device_ids[0] -- evaluation batches are NOT scattered
        over the replicas and gathered back (the default path's ``self.model(img)`` does that); a
        scattered device-side evaluation is not implemented."""
        return self.model.module if (self.distributed or self.data_parallel) else self.model

    def _fused_meters(self, loader, topk: int):
        """The meters of validate() / test() from one on-device evaluation (ResNet.evaluate)."""
        m = self._module_for_eval().evaluate(loader, topk=topk).reference_meters()
        out = []
        for key in ("loss", "top1", "topk"):
            meter = AverageMeter()
            meter.avg = m[key]
            out.append(meter)
        return out

    def _ema_update(self, found_inf) -> None:
        """--model-ema: one update right after the optimizer step, on every --model-ema-steps-th optimizer step (the
        step in progress is optimizer_step + 1; without --accum-steps that is global_step + 1). A GradScaler-skipped
        step updates nothing: the kernel reads `found_inf` on the device."""
        if self.ema is not None and (self.optimizer_step + 1) % self.hparams.model_ema_steps == 0:
            self.ema.update(found_inf=found_inf)

    def validate(self, epoch: int) -> Tuple[float, float]:
        """With --model-ema: the EMA's loss and accuracy (on the device, whatever --fused-eval says), which
        therefore select the best checkpoint; the raw weights' accuracy is kept in ``val_raw_acc`` for the log."""
        if self.ema is None:
            return self._validate_raw(epoch)
        m = self.ema.evaluate(self.val_loader, topk=1).reference_meters()
        self.val_raw_acc = self._validate_raw(epoch)[1]
        return m["loss"], m["top1"]

    def _validate_raw(self, epoch: int) -> Tuple[float, float]:
        if getattr(self.hparams, "fused_eval", False):
            val_loss, top1, _ = self._fused_meters(self.val_loader, 1)
            return val_loss.avg, top1.avg
        val_loss, top1 = AverageMeter(), AverageMeter()
        net = self._module()  # rank 0 evaluates the unwrapped module
        net.eval()
        with torch.no_grad():
            for img, label in self.val_loader:
                img, label = img.to(self.device), label.to(self.device)
                pred = net(img)
                val_loss.update(self.eval_criterion(pred, label).item())
                top1.update(accuracy(pred, label, topk=(1,))[0].item())
        net.train()
        return val_loss.avg, top1.avg

    def test(self, state_dict) -> dict:
        test_loss, top1, top5 = AverageMeter(), AverageMeter(), AverageMeter()
        self.model.load_state_dict(state_dict)
        if getattr(self.hparams, "fused_eval", False):
            test_loss, top1, top5 = self._fused_meters(self.test_loader, 5)
        else:
            net = self._module()
            net.eval()
            with torch.no_grad():
                for img, label in self.test_loader:
                    img, label = img.to(self.device), label.to(self.device)
                    pred = net(img)
                    test_loss.update(self.eval_criterion(pred, label).item())
                    p1, p5 = accuracy(pred, label, topk=(1, 5))
                    top1.update(p1.item())
                    top5.update(p5.item())
        logging.info(f"** Test Loss: {test_loss.avg:.4f}")
        logging.info(f"** Top-1 Accuracy: {top1.avg:.4f}%")
        logging.info(f"** Top-5 Accuracy: {top5.avg:.4f}%")
        return {"test_loss": test_loss.avg, "top_1_acc": top1.avg, "top_5_acc": top5.avg}


def _run(hparams, rank, ngpus, distributed, data_parallel=False):
    D.fix_seed(hparams.seed)
    scaler = GradScaler() if hparams.amp else None
    model = ResNet18()
    if getattr(hparams, "sync_bn", False):
        model = SyncBatchNorm.convert_sync_batchnorm(model)
    trainer = Trainer(hparams, model, scaler, rank, ngpus, distributed, data_parallel)
    trainer.fit()
    if rank == 0 and hparams.contain_test:
        path = glob.glob(os.path.join(trainer.save_path, "best_model_*.pt"))  # (--resume: not under ckpt_path)
        if path:
            state = torch.load(path[0], weights_only=True)
            print(json.dumps(trainer.test(state)))
    return trainer


def main_worker(rank, ngpus_per_node, hparams):
    """ddp/main.py:14-39."""
    hparams.rank = hparams.rank * ngpus_per_node + rank
    torch.cuda.set_device(rank)
    dist.init_process_group(backend=hparams.dist_backend, init_method=hparams.dist_url,
                            world_size=hparams.world_size, rank=hparams.rank)
    try:
        _run(hparams, rank, ngpus_per_node, True)
    finally:
        dist.destroy_process_group()


def main(argv=None, mode: str = "ddp"):
    hparams = load_config(argv, mode)
    if mode == "single":
        return _run(hparams, 0, 1, False)
    if mode == "dp":  # src/dp/main.py: one process, nn.DataParallel over every visible GPU
        return _run(hparams, 0, torch.cuda.device_count(), False, data_parallel=True)
    if mode != "ddp":
        raise ValueError(f"unknown mode {mode!r} (single, dp, ddp)")
    import torch.multiprocessing as mp

    ngpus_per_node = torch.cuda.device_count()
    hparams.world_size = ngpus_per_node * hparams.world_size
    mp.spawn(main_worker, nprocs=ngpus_per_node, args=(ngpus_per_node, hparams))
