"""Whole-image prediction restated in numpy (test infrastructure): the tiling arithmetic, numpy's reflect
padding as an index map, the tile crops, and the stitching of the tiles' cores — around whatever forward the
caller passes (the CPU oracle in tests/test_predict_host.py, the GPU network in tests/test_gpu_predict.py).
Written from the description in DESIGN.md §7f, not from predict.py."""
from __future__ import annotations

import numpy as np
import torch

from oracle import unet_b_cpu as O
from selectivenet_for_semantic_segmentation_binary_amd.data import load_test_set_for_tests
from selectivenet_for_semantic_segmentation_binary_amd.synthetic import make_patches, preprocess

F32 = np.float32


def refl(i, n):
    """numpy 'reflect' padding as an index map onto [0, n): edge not repeated, period 2 (n - 1)."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def grid_of(H, W, tile, halo):
    """(core, (rows, cols), origins [n,2] row-major)."""
    core = tile - 2 * halo
    gy, gx = -(-H // core), -(-W // core)
    origins = np.array([(i * core - halo, j * core - halo) for i in range(gy) for j in range(gx)], np.int64)
    return core, (gy, gx), origins


def crops(image, origins, th, tw):
    """uint8 [n,th,tw,3]: the tiles of the reflect-continued image, by numpy indexing."""
    H, W = image.shape[:2]
    return np.stack([image[refl(y0 + np.arange(th), H)[:, None], refl(x0 + np.arange(tw), W)[None, :]]
                     for y0, x0 in origins])


def stitch(tiles, origins, halo, Hc, Wc, fill=np.nan):
    """fp32 [Hc,Wc]: the cores of tiles [n,th,tw] at (y0 + halo, x0 + halo)."""
    n, th, tw = tiles.shape
    plane = np.full((Hc, Wc), fill, tiles.dtype)
    for t, (y0, x0) in zip(tiles, origins):
        plane[y0 + halo:y0 + th - halo, x0 + halo:x0 + tw - halo] = t[halo:th - halo, halo:tw - halo]
    return plane


def predict_ref(forward, image, tile, halo, batch=None):
    """The whole procedure around `forward(x fp32 [n,3,h,w]) -> (out, sel)` numpy [n,h,w]: the stitched
    (logit, selection) canvases [Hc,Wc]. batch: tiles per forward (None: all at once)."""
    H, W = image.shape[:2]
    core, (gy, gx), origins = grid_of(H, W, tile, halo)
    x, _ = preprocess(crops(image, origins, tile, tile), np.zeros((len(origins), tile, tile), np.uint8))
    batch = batch or len(origins)
    outs = [forward(x[a:a + batch]) for a in range(0, len(origins), batch)]
    out = np.concatenate([o[0] for o in outs])
    sel = np.concatenate([o[1] for o in outs])
    return stitch(out, origins, halo, gy * core, gx * core), stitch(sel, origins, halo, gy * core, gx * core)


def canvas_ref(forward, image, pad, Hc, Wc):
    """One forward of the image reflect-continued over rows [-pad, Hc + pad) and columns [-pad, Wc + pad),
    cut back to the canvas [Hc,Wc]: what tiling with a sufficient halo must reproduce."""
    whole = crops(image, np.array([(-pad, -pad)]), Hc + 2 * pad, Wc + 2 * pad)
    x, _ = preprocess(whole, np.zeros(whole.shape[:3], np.uint8))
    out, sel = forward(x)
    return out[0, pad:pad + Hc, pad:pad + Wc], sel[0, pad:pad + Hc, pad:pad + Wc]


def calibrated_state():
    """The recipe of tests/test_gpu_sweep.py::calibrated_checkpoint: the seed-0 selective state with the
    selection and prediction heads' weights x 64 and each head's bias moved by the median of its oracle
    eval-mode output on the synthetic test fold, so that both heads spread around their thresholds (a fresh
    network's logits span < 0.1). Returns (params, buffers) of the oracle."""
    params, buffers = O.make_state(0, "RGB", True)
    imgs, labs = load_test_set_for_tests("synthetic:8", 64, 2)
    x, _ = preprocess(imgs, labs)
    with torch.no_grad():
        params["conv_select.weight"].mul_(64)
        params["conv1x1.weight"].mul_(64)
        o, s, _ = O.forward(params, buffers, torch.tensor(x), True, training=False)
        params["conv1x1.bias"].sub_(o.median())
        params["conv_select.bias"].sub_(s.median())
    return params, buffers


def state_dict_of(params, buffers):
    sd = {k: v.detach().clone() for k, v in params.items()}
    sd.update({k: v.clone() for k, v in buffers.items()})
    return sd


def oracle_forward(params, buffers):
    def forward(x):
        with torch.no_grad():
            o, s, _ = O.forward(params, buffers, torch.tensor(x), True, training=False)
        return o.numpy(), s.numpy()
    return forward


def sample_image(H=100, W=140, seed=3):
    """An H x W crop of a synthetic patch with a tumor ellipse in it."""
    imgs, _ = make_patches(1, 256, seed=seed, tumorable_frac=1.0)
    return np.ascontiguousarray(imgs[0, :H, :W])
