"""Prioritization orders: Coverage-Total (CTM) and Coverage-Additional (CAM).

API parity with reference src/core/prioritizers.py:7-59 (generators yielding
indices), implemented over packed bitmaps so the CAM greedy set-cover loop can
run device-resident on MI355X (ops.cam_order)."""

from typing import Generator, List, Sequence, Union

import numpy as np
import torch

from .. import ops
from .bitmap import BitProfile


def _as_tensor(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x
    return torch.as_tensor(np.asarray(x))


def ctm(scores) -> Generator[int, None, None]:
    """Indices by decreasing score (Coverage-Total Method)."""
    scores = _as_tensor(scores)
    assert scores.dim() == 1
    for x in ops.ctm_order(scores).cpu().tolist():
        yield x


def cam(scores, profiles: Union[BitProfile, torch.Tensor, np.ndarray]) -> Generator[int, None, None]:
    """Indices by greedily maximising added coverage (Coverage-Additional).

    ``profiles`` may be a :class:`BitProfile` or a bool matrix (higher-rank
    inputs are flattened per sample, like the reference).
    """
    scores = _as_tensor(scores).float()
    profiles = _as_profile(profiles)
    order = ops.cam_order(scores, profiles.words, profiles.nbits)
    for x in order.cpu().tolist():
        yield x


def _as_profile(profiles) -> BitProfile:
    if not isinstance(profiles, BitProfile):
        p = _as_tensor(profiles)
        p = p.reshape(p.shape[0], -1).bool()
        profiles = BitProfile.from_bool(p)
    return profiles


def cam_many(scores_list: Sequence, profiles_list: Sequence) -> List[List[int]]:
    """The :func:`cam` orders of several independent (scores, profiles)
    pairs, as lists, from one batched call (ops.cam_order_many): on the GPU
    one persistent launch orders up to ``ops.cam_many_max_problems()`` of
    them side by side. Each entry of ``profiles_list`` may be a
    :class:`BitProfile` or a bool matrix, like ``cam``'s; entry ``p`` of the
    result equals ``list(cam(scores_list[p], profiles_list[p]))``.
    """
    scores_list, profiles_list = list(scores_list), list(profiles_list)
    if len(scores_list) != len(profiles_list):
        raise ValueError("cam_many needs one profile per score vector")
    profiles = [_as_profile(p) for p in profiles_list]
    scores = [
        _as_tensor(s).float().to(p.words.device)
        for s, p in zip(scores_list, profiles)
    ]
    orders = ops.cam_order_many(
        scores,
        [p.words.contiguous() for p in profiles],
        [p.nbits for p in profiles],
    )
    return [o.cpu().tolist() for o in orders]
