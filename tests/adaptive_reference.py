"""The adaptive anti-aliasing contract (include/portal_amd.h) restated in numpy.  Integers only.

    d(x, y)      = max over dx, dy in {-1, 0, 1}, c in {R, G, B} of | P(clamp(x+dx), clamp(y+dy)).c - P(x, y).c |
    refine(x, y) = d(x, y) > T
    out(x, y)    = refine(x, y) ? F(x, y) : P(x, y)

P: the RGBA8 frame drawn with one sample per pixel, F: the frame drawn with the full `aa_count`, T: an integer in -1 .. 255.
Coordinates clamp to the frame, alpha is ignored.

Behind the contract: the small helpers tests/test_adaptive_aa.py and tests/test_adaptive_slices.py share.
"""
import os
import re

import numpy as np


def distance(p: np.ndarray) -> np.ndarray:
    """d of every pixel of an H x W x 4 uint8 frame, as an H x W int32 array."""
    assert p.dtype == np.uint8 and p.ndim == 3 and p.shape[2] == 4
    h, w = p.shape[:2]
    rgb = p[:, :, :3].astype(np.int32)
    ys, xs = np.arange(h), np.arange(w)
    d = np.zeros((h, w), np.int32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near = rgb[np.clip(ys + dy, 0, h - 1)][:, np.clip(xs + dx, 0, w - 1)]
            d = np.maximum(d, np.abs(near - rgb).max(axis=2))
    return d


def refine_mask(p: np.ndarray, threshold: int) -> np.ndarray:
    assert -1 <= int(threshold) <= 255
    return distance(p) > int(threshold)


def refined_indices(p: np.ndarray, threshold: int) -> np.ndarray:
    """The sorted pixel indices y * W + x of the refined pixels (the GPU's list is free in its order)."""
    return np.flatnonzero(refine_mask(p, threshold)).astype(np.uint32)


def adaptive_frame(p: np.ndarray, f: np.ndarray, threshold: int) -> np.ndarray:
    """out for frames of any per-pixel payload (RGBA8 bytes, or the RGBA32F bits as uint32) classified on the RGBA8 frame `p`."""
    return select(refine_mask(p, threshold), f, p)


def select(mask: np.ndarray, f: np.ndarray, p: np.ndarray) -> np.ndarray:
    assert mask.shape == f.shape[:2] == p.shape[:2]
    return np.where(mask[:, :, None], f, p)


# ---- shared by the two test files -------------------------------------------------------------------
def resource_usage(stderr):
    """hipcc -Rpass-analysis=kernel-resource-usage -> {kernel: {"VGPRs" | "ScratchSize [bytes/lane]" | "LDS Size [bytes/block]": value}}."""
    usage, name = {}, None
    for line in stderr.splitlines():
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs): (\d+)", line)
        if m and name:
            usage.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return usage


def exe(pa):
    return os.path.join(os.path.dirname(pa.__file__), "portal-amd")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cuda_words(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()
