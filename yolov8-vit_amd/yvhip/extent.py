"""The extent of a detector input: an int (a square) or an (H, W) pair.  Host arithmetic only: needs no GPU."""
from __future__ import annotations

from typing import Tuple

from . import YvError


def net_hw(size) -> Tuple[int, int]:
    """(H, W) of a network extent given as an int (square) or an (H, W) pair; both sides positive multiples of 32, else
    YvError."""
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise YvError("input size must be an int or an (H, W) pair")
        H, W = int(size[0]), int(size[1])
    else:
        H = W = int(size)
    if H <= 0 or W <= 0 or H % 32 or W % 32:
        raise YvError("input size must be a multiple of 32")
    return H, W


def n_anchors(H: int, W: int) -> int:
    """Anchors of an H x W network input: scales 8, 16, 32 concatenated."""
    return sum((H // s) * (W // s) for s in (8, 16, 32))
