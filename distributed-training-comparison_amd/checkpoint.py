"""Full training checkpoints: everything a run needs to continue bit for bit from an epoch boundary.

``capture`` gathers the state of the model (weights, running statistics, batch counts), the fused optimizer (its
flat state buffers in torch's per-parameter format), the GradScaler, the weight EMA with its update count, the LR
scheduler and the four random generators (``torch``, ``torch.cuda`` of the current device, ``numpy``, ``random``)
into one dict of contiguous CPU tensors and plain values; ``restore`` puts it back, the generators last. ``save``
writes atomically; ``load`` reads with ``weights_only=True``, so a file holds only dicts, lists, tuples, tensors,
numbers, strings, bytes and None -- never a pickled object. No kernel is involved: a checkpoint is a few
device-to-host copies at an epoch boundary.
"""
from __future__ import annotations

import os
import pickle
import random

import numpy as np
import torch

FORMAT_KEY = "dtc_checkpoint"
FORMAT = 1


class CheckpointError(RuntimeError):
    """A checkpoint that cannot be read, or that does not fit the run it is loaded into."""


def to_plain(obj, where: str = "state"):
    """`obj` with every tensor as a contiguous CPU copy, every mapping as a dict, numpy scalars as Python numbers.
    Anything ``load`` could not read back (an object, a function) is refused with its place in the tree."""
    if isinstance(obj, torch.Tensor):
        return obj.detach().to("cpu", copy=True).contiguous()
    if obj is None or isinstance(obj, (bool, int, float, str, bytes)):
        return obj
    if isinstance(obj, np.generic):
        return obj.item()
    if isinstance(obj, dict):
        for k in obj:
            if not isinstance(k, (int, str)):
                raise TypeError(f"checkpoint: the key {k!r} of {where} is neither a string nor an integer")
        return {k: to_plain(v, f"{where}[{k!r}]") for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        items = [to_plain(v, f"{where}[{i}]") for i, v in enumerate(obj)]
        return tuple(items) if isinstance(obj, tuple) else items
    raise TypeError(f"checkpoint: {where} is a {type(obj).__name__}, which a checkpoint file cannot hold")


def get_rng_state() -> dict:
    """The states of the four generators as tensors, lists and numbers. Reads only: no random number is drawn."""
    name, keys, pos, has_gauss, cached = np.random.get_state()
    version, words, gauss_next = random.getstate()
    cuda = None
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        cuda = torch.cuda.get_rng_state(torch.cuda.current_device()).clone()
    return {"torch": torch.get_rng_state().clone(), "cuda": cuda,
            "numpy": {"name": str(name), "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos),
                      "has_gauss": int(has_gauss), "cached_gaussian": float(cached)},
            "random": {"version": int(version), "words": [int(w) for w in words], "gauss_next": gauss_next}}


def set_rng_state(state: dict) -> None:
    torch.set_rng_state(state["torch"])
    if state.get("cuda") is not None and torch.cuda.is_available():
        torch.cuda.set_rng_state(state["cuda"], torch.cuda.current_device())
    n = state["numpy"]
    np.random.set_state((n["name"], n["keys"].numpy().astype(np.uint32), n["pos"], n["has_gauss"],
                         n["cached_gaussian"]))
    r = state["random"]
    random.setstate((r["version"], tuple(r["words"]), r["gauss_next"]))


def capture(model, optimizer, scaler=None, ema=None, scheduler=None, extra=None) -> dict:
    """The training state as one dict of CPU copies (the device is synchronised by the copies). Nothing that
    changes the training state is launched and no random number is consumed. `extra`: the caller's own record
    (epoch, step counts, ...), returned by ``restore``."""
    return {FORMAT_KEY: FORMAT,
            "model": to_plain(dict(model.state_dict()), "model"),
            "optimizer": to_plain(optimizer.state_dict(), "optimizer"),
            "scaler": None if scaler is None else to_plain(scaler.state_dict(), "scaler"),
            "ema": None if ema is None else to_plain(ema.train_state(), "ema"),
            "scheduler": None if scheduler is None else to_plain(scheduler.state_dict(), "scheduler"),
            "extra": to_plain(extra, "extra"),
            "rng": get_rng_state()}


def restore(state: dict, model, optimizer, scaler=None, ema=None, scheduler=None):
    """Put ``capture``'s dict back into freshly built objects and return its `extra`. A part the state holds but
    the run lacks, or the other way round, is refused (optimizer against model is checked by the optimizer). The
    random generators are restored last: whatever was built or loaded before has drawn what it draws."""
    _check_format(state, "the state")
    for name, obj in (("scaler", scaler), ("ema", ema), ("scheduler", scheduler)):
        if (obj is None) != (state.get(name) is None):
            raise CheckpointError(f"checkpoint: the state {'holds no' if obj is not None else 'holds a'} {name} but "
                                  f"this run {'has one' if obj is not None else 'has none'}")
    model.load_state_dict(state["model"])
    optimizer.load_state_dict(state["optimizer"])
    if scaler is not None:
        scaler.load_state_dict(state["scaler"])
    if ema is not None:
        ema.load_train_state(state["ema"])
    if scheduler is not None:
        scheduler.load_state_dict(dict(state["scheduler"]))
    set_rng_state(state["rng"])
    return state.get("extra")


def _check_format(state, what: str) -> None:
    tag = state.get(FORMAT_KEY) if isinstance(state, dict) else None
    if tag != FORMAT:
        raise CheckpointError(f"checkpoint: {what} has the format tag {FORMAT_KEY!r} = {tag!r}, expected {FORMAT}")


def save(path: str, state: dict) -> None:
    """Write `state` to `path` through ``path + ".tmp"`` and ``os.replace``: a writer killed half-way leaves the
    previous file under the real name, never a truncated one."""
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        torch.save(state, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def load(path: str) -> dict:
    """Read a file ``save`` wrote, onto the CPU, with ``weights_only=True`` (a file holding a pickled object is
    refused); a file without the format tag, or with another one, is refused too."""
    try:
        state = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        raise CheckpointError(f"checkpoint: {path} holds more than tensors and plain values: {e}") from e
    _check_format(state, path)
    return state
