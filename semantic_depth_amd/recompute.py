"""Bookkeeping of the per-frame fp16 range recompute (Engine(on_range="recompute")).

The engine reads the per-frame clamp counts of a call (sd_saturation_frames), recomputes the flagged frames on a companion bf16x3 engine
and splices those frames' results into its own outputs.  The functions here hold no engine state and accept CPU or device tensors, so
the splice is tested without a GPU.  Every output of a call is batch-major ([B, ...] per frame), so a splice is one index_copy_ per
tensor on the tensors' own device: clouds, records and masks never pass through the host.
"""
from __future__ import annotations

import numpy as np
import torch

ON_RANGE_MODES = ("raise", "recompute")


def check_mode(on_range: str) -> str:
    if on_range not in ON_RANGE_MODES:
        raise ValueError(f"on_range must be one of {ON_RANGE_MODES}, not {on_range!r}")
    return on_range


def flagged_frames(counts) -> list[int]:
    """indices of the frames with a non-zero clamp count, ascending"""
    return [int(i) for i in np.flatnonzero(np.asarray(counts))]


def splice(dst, src, index: torch.Tensor):
    """write frame j of ``src`` over frame index[j] of ``dst``, in place, for every tensor of the (nested) result.

    ``dst`` / ``src`` are tensors, dicts, tuples / lists of them or None; a dict is walked over the keys of ``dst`` (``src`` may hold
    more: a subset that fits one network pass returns the fused disparity beside the clouds).  ``dst`` entries that are None stay None;
    a tensor of ``dst`` must have its match in ``src`` with the same trailing shape.  Returns ``dst``."""
    if dst is None:
        return None
    if isinstance(dst, torch.Tensor):
        if not isinstance(src, torch.Tensor):
            raise TypeError(f"splice: no tensor to splice into a {tuple(dst.shape)} output")
        if src.shape[0] != index.numel() or tuple(src.shape[1:]) != tuple(dst.shape[1:]) or src.dtype != dst.dtype:
            raise ValueError(f"splice: {src.dtype} {tuple(src.shape)} for {index.numel()} frames of {dst.dtype} {tuple(dst.shape)}")
        dst.index_copy_(0, index.to(dst.device), src.to(dst.device))
        return dst
    if isinstance(dst, dict):
        for k, v in dst.items():
            if v is not None:
                if k not in src:
                    raise KeyError(f"splice: the recomputed result has no {k!r}")
                splice(v, src[k], index)
        return dst
    if isinstance(dst, (tuple, list)):
        if len(dst) != len(src):
            raise ValueError("splice: results of different structure")
        for a, b in zip(dst, src):
            splice(a, b, index)
        return dst
    raise TypeError(f"splice: cannot splice a {type(dst).__name__}")
