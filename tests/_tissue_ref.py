"""The tissue mask of whole-image prediction restated in numpy (test infrastructure), on top of
tests/_predict_ref.py and tests/_tta_ref.py: the pixel rule, the tissue counts of the tiles' input windows, the
glass model, the fixed half-glass image and the kept tiles of every ensemble member. Written from the
description in DESIGN.md §7i, not from predict.py."""
from __future__ import annotations

import numpy as np

from tests import _predict_ref as R
from tests import _tta_ref as TR

BRIGHT, SPREAD = 237, 11  # floor(255 (0.96 - 6 * 0.005)), ceil(255 * 6 * sqrt(2) * 0.005)
TILE, HALO = 160, 56


def plane_of(image, bright=BRIGHT, spread=SPREAD):
    """uint8 [H,W]: 0 where min(r,g,b) >= bright and max - min <= spread (glass), 255 elsewhere (tissue)."""
    px = image.astype(np.int64)
    lo, hi = px.min(axis=2), px.max(axis=2)
    return np.where((lo >= bright) & (hi - lo <= spread), 0, 255).astype(np.uint8)


def window_counts(plane, origins, th, tw, flip=0):
    """int64 [n]: the tissue pixels of each tile's th x tw window of the plane flipped by `flip` (bit 1 rows, bit
    0 columns) and continued by reflection: a reflected copy counts again."""
    flipped = TR.T(flip & 3, plane)
    H, W = flipped.shape
    return np.array([np.count_nonzero(flipped[R.refl(y0 + np.arange(th), H)[:, None], R.refl(x0 + np.arange(tw), W)[None, :]])
                     for y0, x0 in origins], np.int64)


def glass(shape, seed):
    """The glass model as uint8: 0.96 + 0.005 N(0,1) per channel, clipped to [0, 1], rounded to a level."""
    return np.floor(255 * np.clip(0.96 + 0.005 * np.random.default_rng(seed).standard_normal(shape), 0, 1) + 0.5).astype(np.uint8)


def fixed_image():
    """200 x 296: a synthetic patch on the left, glass on the right with one speck of tissue at (10, 250)."""
    image = np.concatenate([R.sample_image(200, 148, seed=3), glass((200, 148, 3), 1)], axis=1)
    image[10, 250] = (120, 40, 130)
    return np.ascontiguousarray(image)


def kept_of(image, member, min_pixels=1, tile=TILE, halo=HALO, bright=BRIGHT, spread=SPREAD):
    """bool [n]: the tiles member k = 4 c + f forwards, over the tiling of its own orientation class c."""
    src = TR.T(member & 4, image)
    _, _, origins = R.grid_of(src.shape[0], src.shape[1], tile, halo)
    return window_counts(plane_of(src, bright, spread), origins, tile, tile, member & 3) >= min_pixels


def core_cover(shape, kept, tile=TILE, halo=HALO):
    """bool [H,W]: the pixels of an H x W image that lie in the core of a kept tile."""
    H, W = shape
    core, (gy, gx), _ = R.grid_of(H, W, tile, halo)
    return np.kron(np.asarray(kept).reshape(gy, gx), np.ones((core, core), bool))[:H, :W].astype(bool)
