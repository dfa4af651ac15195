"""Whole-image prediction (MI355X path only; the reference has no such tool: its eval.py keeps
`make_heatmap` with the saving code commented out): a trained UNet_B applied to an RGB image of any size,
unlabelled, giving a tumor / abstained / background mask, a probability map and the logit planes.

    python -m selectivenet_for_semantic_segmentation_binary_amd.predict --input slide_region.png more/ \\
        --model_dir /model/1-fold/checkpoint --model_arch UNet_B --selective 1 --save_dir ./output

The network is fully convolutional in eval mode (BatchNorm uses its running statistics), so the image is
cut into overlapping tiles (`TilePlan`): each tile is gathered from the uint8 image on the device, the image
continued past its edges by reflection (`selunet_tile_gather`), run through the forward, and its core — the
tile minus a halo on every side — stitched into the canvases (`selunet_tile_stitch`). An output pixel
depends on input pixels at most 51 away, so with a halo of at least HALO_MIN = 56 that is a
multiple of 8 (the three 2x2 poolings see every tile on the grid of the whole image) the stitched planes are
those of one forward of the whole reflect-padded image. The image is uploaded once, and nothing is read
back before the end.

Per input the CLI writes `<stem>_mask.png` (L: 0 background, 127 abstained, 255 tumor), `<stem>_prob.png`
(L: round(255 sigmoid(logit))) and, with a selective network, `<stem>_select.png` (L: 255 where selected),
and for the run `predict.json`: per image its size, the tile grid, the pixel counts, the tumor fraction of
the selected pixels and the coverage. Thresholds are `metrics.logit_threshold(rule="eval")`, as eval's.

`--tta flips` / `--tta d4` (`predict_image(..., tta=)`) averages the logit planes of the 4 flips / the 8 flips and
transposes of the image on the device; the mask, the probability map and the counts then come from
the means, `<stem>_votes.png` (L: votes * 255 // members) shows how many orientations say tumor, and predict.json
carries "tta" and per image "unanimous_fraction", the share of pixels on which all orientations agree.

`--regions 1`, `--min_region N`, `--fill_holes M`, `--connectivity {4,8}` (`predict_image(..., regions=, min_region=,
fill_holes=, connectivity=)`) label the tumor regions of the mask on the device, remove regions of fewer
than N pixels, fill enclosed background holes of at most M pixels that touch no abstained pixel, and report the
regions of the cleaned mask: `<stem>_mask.png` is then the cleaned mask, `<stem>_regions.csv` holds one row per region
(exact integer columns plus centroid and mean probability), and the image's predict.json entry gains "regions",
"largest_region_area" and "cleanup". Without these flags nothing of that runs and every file is as before.

`--tissue 1`, `--tissue_bright B`, `--tissue_spread S`, `--tissue_min_pixels N` (`predict_image(..., tissue=, tissue_bright=,
tissue_spread=, tissue_min_pixels=)`) mark bare glass on the device (a pixel is glass iff min(r,g,b) >= B
and max - min <= S) and do not forward a tile whose input window holds fewer than N tissue pixels: its core is background,
selected, with logit -inf and prob8 0. `<stem>_tissue.png` (L: 255 tissue, 0 glass) is written, the image's predict.json
entry gains "tissue_pixels", "tissue_counts", "tumor_fraction_of_tissue", "tiles_forwarded" and "tiles_total", and the
document's head the rule's three numbers. Without `--tissue 1` nothing of that runs and every file is as before.

`--stain_norm macenko`, `--stain_target FILE.json`, `--stain_beta B` (`predict_image(..., stain=, stain_beta=)`; DESIGN.md
§7m) bring the image to the stain vectors and strengths of a target before it is tiled: a Macenko fit and re-rendering on
the device, once per image (stain.py). The target is the published default or, better, the checkpoint's own training stain
made by `python -m selectivenet_for_semantic_segmentation_binary_amd.stain fit`. The tissue plane of `--tissue` is still that
of the original image. `<stem>_stain.png` is the normalised image, the image's predict.json entry gains "stain" (applied,
reason, the fitted HE and maxC, n_stained, skipped, T) and the document's head the method, the target and beta. Where nothing
can be fitted the image is predicted as it is and "applied" is false. Without the flag nothing of that runs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as K
from . import metrics as MT
from . import stain as ST
from .data import _CIN, _MODE

HALO_MIN = 56   # the receptive field reaches 51 pixels to either side; the next multiple of 8
TILE_MAX = 512  # the largest forward the engine is tested at is 512 x 512
IMAGE_MAX = 65535
IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".tif", ".tiff", ".bmp")
COUNT_NAMES = ("background", "tumor", "abstained", "pixels")
TTA_MEMBERS = {"none": 1, "flips": 4, "d4": 8}  # members of the test-time-augmentation ensemble


class TilePlan:
    """The tiling of an H x W image: square tiles of `tile` pixels whose cores of `core = tile - 2 halo`
    pixels cover the canvas `Hc x Wc = grid * core >= H x W` exactly once. `origins` (int32 [n][2], row-major
    over the grid) holds each tile's (y0, x0) = (i core - halo, j core - halo) in image coordinates: negative
    in the first row and column, and the last ones reach past the image."""

    def __init__(self, H: int, W: int, tile: int = 512, halo: int = HALO_MIN, allow_small_halo: bool = False):
        H, W, tile, halo = int(H), int(W), int(tile), int(halo)
        if not (1 <= H <= IMAGE_MAX and 1 <= W <= IMAGE_MAX):
            raise ValueError(f"TilePlan: image height and width must be in [1, {IMAGE_MAX}] (got {H} x {W})")
        if halo < 0 or halo % 8 != 0:
            raise ValueError(f"TilePlan: halo {halo} must be a multiple of 8 (the poolings of every tile must lie on "
                             "the grid of the whole image)")
        if halo < HALO_MIN and not allow_small_halo:
            raise ValueError(f"TilePlan: halo {halo} is below HALO_MIN = {HALO_MIN}: an output pixel sees input up to "
                             "51 pixels away, so the stitched result would depend on the tiling")
        if tile % 8 != 0:
            raise ValueError(f"TilePlan: tile {tile} must be a multiple of 8")
        if tile <= 2 * halo:
            raise ValueError(f"TilePlan: tile {tile} leaves no core inside a halo of {halo} (tile must exceed 2 halo)")
        if tile > TILE_MAX:
            raise ValueError(f"TilePlan: tile {tile} is above {TILE_MAX}: the engine has no fixture above "
                             f"{TILE_MAX} x {TILE_MAX}, so larger forwards are untested")
        self.H, self.W, self.tile, self.halo = H, W, tile, halo
        self.core = tile - 2 * halo
        self.grid = (-(-H // self.core), -(-W // self.core))
        self.Hc, self.Wc = self.grid[0] * self.core, self.grid[1] * self.core
        ij = np.indices(self.grid).reshape(2, -1).T  # row-major (i, j)
        self.origins = np.ascontiguousarray(ij * self.core - halo, dtype=np.int32)

    @property
    def n(self) -> int:
        return len(self.origins)

    def __repr__(self):
        return (f"TilePlan({self.H} x {self.W}: {self.grid[0]} x {self.grid[1]} tiles of {self.tile}, halo "
                f"{self.halo}, canvas {self.Hc} x {self.Wc})")


def _check(name, t, dtype):
    if t is not None and (not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != dtype
                          or not t.is_contiguous()):
        raise RuntimeError(f"{name} must be a contiguous cuda {dtype} tensor")


def tile_gather(image_u8: torch.Tensor, origins: torch.Tensor, th: int, tw: int, input_type: str = "RGB",
                out: torch.Tensor | None = None) -> torch.Tensor:
    """`selunet_tile_gather`: image uint8 [H,W,3] and origins int32 [n,2], both on the GPU -> x fp32
    [n,C,th,tw] (into `out` when given)."""
    if input_type not in _MODE:
        raise ValueError(f"input_type {input_type!r}: 'RGB', 'GH' or 'H_RGB'")
    _check("tile_gather: image", image_u8, torch.uint8)
    _check("tile_gather: origins", origins, torch.int32)
    if image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise ValueError(f"tile_gather: image must be RGB [H,W,3] uint8 (got {tuple(image_u8.shape)})")
    if origins.dim() != 2 or origins.shape[1] != 2:
        raise ValueError(f"tile_gather: origins must be [n,2] (got {tuple(origins.shape)})")
    n, shape = origins.shape[0], (origins.shape[0], _CIN[input_type], th, tw)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=image_u8.device)
    _check("tile_gather: out", out, torch.float32)
    if tuple(out.shape) != shape:
        raise ValueError(f"tile_gather: out must be {shape} (got {tuple(out.shape)})")
    K.call("selunet_tile_gather", K.ptr(image_u8), image_u8.shape[0], image_u8.shape[1], K.ptr(origins), n, th, tw,
           _MODE[input_type], K.ptr(out), K.stream_ptr())
    return out


def tile_stitch(out: torch.Tensor, sel: torch.Tensor | None, origins_host: np.ndarray, origins: torch.Tensor,
                halo: int, H: int, W: int, t_out: float, t_sel: float, logit_plane: torch.Tensor,
                sel_plane: torch.Tensor | None, mask: torch.Tensor, prob8: torch.Tensor | None,
                counts: torch.Tensor):
    """`selunet_tile_stitch`: the cores of the output tiles out / sel [n,th,tw] into the canvases [Hc,Wc].
    `origins_host` is the host copy of the device `origins`: the library never reads the device array on the
    host, so the rule it cannot check — every core inside the canvas, at a column that is a multiple of 8 — is
    checked here."""
    _check("tile_stitch: out", out, torch.float32)
    _check("tile_stitch: sel", sel, torch.float32)
    _check("tile_stitch: origins", origins, torch.int32)
    _check("tile_stitch: logit_plane", logit_plane, torch.float32)
    _check("tile_stitch: sel_plane", sel_plane, torch.float32)
    _check("tile_stitch: mask", mask, torch.uint8)
    _check("tile_stitch: prob8", prob8, torch.uint8)
    _check("tile_stitch: counts", counts, torch.int64)
    if out.dim() != 3 or (sel is not None and sel.shape != out.shape):
        raise ValueError("tile_stitch: out and sel must be [n,th,tw] of one shape")
    n, th, tw = out.shape
    oh = np.asarray(origins_host)
    if oh.shape != (n, 2) or tuple(origins.shape) != (n, 2):
        raise ValueError(f"tile_stitch: origins must be [{n},2] on the host and on the device")
    if logit_plane.dim() != 2 or counts.numel() != 4:
        raise ValueError("tile_stitch: logit_plane must be [Hc,Wc] and counts hold 4 words")
    Hc, Wc = logit_plane.shape
    for name, t in (("sel_plane", sel_plane), ("mask", mask), ("prob8", prob8)):
        if t is not None and tuple(t.shape) != (Hc, Wc):
            raise ValueError(f"tile_stitch: {name} must be [{Hc},{Wc}] like logit_plane (got {tuple(t.shape)})")
    _check_cores("tile_stitch", oh, n, th, tw, halo, Hc, Wc)
    K.call("selunet_tile_stitch", K.ptr(out), K.ptr(sel), K.ptr(origins), n, th, tw, halo, H, W, Hc, Wc, t_out, t_sel,
           K.ptr(logit_plane), K.ptr(sel_plane), K.ptr(mask), K.ptr(prob8), K.ptr(counts), K.stream_ptr())


def _check_cores(fn, origins_host, n, th, tw, halo, Hc, Wc):
    """The rule the library cannot check (the origins live on the device), on their host copy: every core
    inside the Hc x Wc canvas at a column that is a multiple of 8."""
    oh = np.asarray(origins_host)
    if oh.shape != (n, 2):
        raise ValueError(f"{fn}: origins must be [{n},2] on the host and on the device")
    cy, cx = oh[:, 0].astype(np.int64) + halo, oh[:, 1].astype(np.int64) + halo
    if 0 <= 2 * halo < min(th, tw) and (
            (cy < 0).any() or (cx < 0).any() or (cy + th - 2 * halo > Hc).any() or (cx + tw - 2 * halo > Wc).any()
            or (cx % 8 != 0).any()):
        raise K.SelunetError(f"selunet_{fn}: a tile's core does not lie inside the {Hc} x {Wc} canvas at a "
                             "column that is a multiple of 8")


def tile_gather_flip(image_u8: torch.Tensor, origins: torch.Tensor, th: int, tw: int, input_type: str = "RGB",
                     flip: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """`selunet_tile_gather_flip`: `tile_gather` of the image with its rows (flip & 2) and columns (flip & 1)
    reversed, without forming that image."""
    if input_type not in _MODE:
        raise ValueError(f"input_type {input_type!r}: 'RGB', 'GH' or 'H_RGB'")
    _check("tile_gather_flip: image", image_u8, torch.uint8)
    _check("tile_gather_flip: origins", origins, torch.int32)
    if image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise ValueError(f"tile_gather_flip: image must be RGB [H,W,3] uint8 (got {tuple(image_u8.shape)})")
    if origins.dim() != 2 or origins.shape[1] != 2:
        raise ValueError(f"tile_gather_flip: origins must be [n,2] (got {tuple(origins.shape)})")
    n, shape = origins.shape[0], (origins.shape[0], _CIN[input_type], th, tw)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=image_u8.device)
    _check("tile_gather_flip: out", out, torch.float32)
    if tuple(out.shape) != shape:
        raise ValueError(f"tile_gather_flip: out must be {shape} (got {tuple(out.shape)})")
    K.call("selunet_tile_gather_flip", K.ptr(image_u8), image_u8.shape[0], image_u8.shape[1], K.ptr(origins), n, th,
           tw, _MODE[input_type], int(flip), K.ptr(out), K.stream_ptr())
    return out


def image_transpose(image_u8: torch.Tensor) -> torch.Tensor:
    """`selunet_image_transpose`: uint8 [H,W,3] on the GPU -> a new [W,H,3]."""
    _check("image_transpose: image", image_u8, torch.uint8)
    if image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise ValueError(f"image_transpose: image must be RGB [H,W,3] uint8 (got {tuple(image_u8.shape)})")
    H, W = image_u8.shape[:2]
    out = torch.empty(W, H, 3, dtype=torch.uint8, device=image_u8.device)
    K.call("selunet_image_transpose", K.ptr(image_u8), H, W, K.ptr(out), K.stream_ptr())
    return out


def tta_accumulate(out: torch.Tensor, sel: torch.Tensor | None, origins_host: np.ndarray, origins: torch.Tensor,
                   halo: int, flip: int, first: bool, H: int, W: int, Hc: int, Wc: int, t_out: float, t_sel: float,
                   sum_out: torch.Tensor, sum_sel: torch.Tensor | None, votes: torch.Tensor,
                   sel_votes: torch.Tensor | None):
    """`selunet_tta_accumulate`: the cores of one member's output tiles out / sel [n,th,tw], flipped back by
    `flip`, into the sums and votes [H,ws] of the member's orientation class (`first`: stored, not added).
    H x W is the member's image and Hc x Wc its plan's canvas; `origins_host` as `tile_stitch`'s."""
    _check("tta_accumulate: out", out, torch.float32)
    _check("tta_accumulate: sel", sel, torch.float32)
    _check("tta_accumulate: origins", origins, torch.int32)
    _check("tta_accumulate: sum_out", sum_out, torch.float32)
    _check("tta_accumulate: sum_sel", sum_sel, torch.float32)
    _check("tta_accumulate: votes", votes, torch.uint8)
    _check("tta_accumulate: sel_votes", sel_votes, torch.uint8)
    if out.dim() != 3 or (sel is not None and sel.shape != out.shape):
        raise ValueError("tta_accumulate: out and sel must be [n,th,tw] of one shape")
    n, th, tw = out.shape
    if tuple(origins.shape) != (n, 2):
        raise ValueError(f"tta_accumulate: origins must be [{n},2] on the host and on the device")
    if sum_out.dim() != 2 or sum_out.shape[0] < H:
        raise ValueError(f"tta_accumulate: sum_out must be [>= {H}, ws] (got {tuple(sum_out.shape)})")
    for name, t in (("sum_sel", sum_sel), ("votes", votes), ("sel_votes", sel_votes)):
        if t is not None and t.shape != sum_out.shape:
            raise ValueError(f"tta_accumulate: {name} must be {tuple(sum_out.shape)} like sum_out (got {tuple(t.shape)})")
    _check_cores("tta_accumulate", origins_host, n, th, tw, halo, Hc, Wc)
    K.call("selunet_tta_accumulate", K.ptr(out), K.ptr(sel), K.ptr(origins), n, th, tw, halo, int(flip), int(first),
           H, W, sum_out.shape[1], t_out, t_sel, K.ptr(sum_out), K.ptr(sum_sel), K.ptr(votes), K.ptr(sel_votes),
           K.stream_ptr())


def tta_finalize(a, b, members: int, H: int, W: int, t_out: float, t_sel: float, prob8: bool = True):
    """`selunet_tta_finalize`. a = (sum_out, sum_sel | None, votes, sel_votes | None), each [H,wa]: the class of
    members 0..3; b: the same for members 4..7, each [W,hb], or None for 4 members. Returns (logit, selection |
    None, mask, prob8 | None, votes, sel_votes | None), each [H,wa], and the device counts (int64 [4])."""
    kinds = (torch.float32, torch.float32, torch.uint8, torch.uint8)
    for name, group in (("a", a), ("b", b)):
        for t, dt in zip(group or (), kinds):
            _check(f"tta_finalize: {name}", t, dt)
            if t is not None and t.shape != group[0].shape:
                raise ValueError(f"tta_finalize: the planes of {name} must be of one shape")
    if a[0].dim() != 2 or a[0].shape[0] < H or (b is not None and (b[0].dim() != 2 or b[0].shape[0] < W)):
        raise ValueError("tta_finalize: a must be [>= H, wa] and b [>= W, hb]")
    selective = a[1] is not None
    dev = a[0].device
    new = lambda dt: torch.zeros(H, a[0].shape[1], dtype=dt, device=dev)  # noqa: E731
    logit, mask, votes = new(torch.float32), new(torch.uint8), new(torch.uint8)
    selection, sel_votes = (new(torch.float32), new(torch.uint8)) if selective else (None, None)
    prob = new(torch.uint8) if prob8 else None
    counts = torch.zeros(4, dtype=torch.int64, device=dev)  # uint64 bits
    b = b or (None,) * 4
    K.call("selunet_tta_finalize", *[K.ptr(t) for t in a], *[K.ptr(t) for t in b], members, H, W, a[0].shape[1],
           0 if b[0] is None else b[0].shape[1], t_out, t_sel, K.ptr(logit), K.ptr(selection), K.ptr(mask),
           K.ptr(prob), K.ptr(votes), K.ptr(sel_votes), K.ptr(counts), K.stream_ptr())
    return (logit, selection, mask, prob, votes, sel_votes), counts


# ----------------------------------------------------------------------------- tissue
# The reference's glass model paints 0.96 + 0.005 N(0,1) per channel (utils/data_utils.py:127-157); the defaults
# are that model at six standard deviations: bright = floor(255 (0.96 - 6 * 0.005)), spread = ceil(255 * 6 *
# sqrt(2) * 0.005) (the difference of two channels has sqrt(2) times a channel's deviation).
TISSUE_BRIGHT = 237
TISSUE_SPREAD = 11


def _tissue_args(fn, bright, spread, min_pixels):
    for name, v in (("tissue_bright", bright), ("tissue_spread", spread)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= v <= 255:
            raise ValueError(f"{fn}: {name} must be an integer in [0, 255] (got {v!r})")
    if not isinstance(min_pixels, (int, np.integer)) or isinstance(min_pixels, bool) or min_pixels < 1:
        raise ValueError(f"{fn}: tissue_min_pixels must be an integer >= 1 (got {min_pixels!r})")


def tissue_plane(image_u8: torch.Tensor, bright: int = TISSUE_BRIGHT, spread: int = TISSUE_SPREAD) -> torch.Tensor:
    """`selunet_tissue_plane`: image uint8 [H,W,3] on the GPU -> uint8 [H,W], 255 tissue / 0 glass (glass iff
    min(r,g,b) >= bright and max - min <= spread): a view of a plane whose rows are padded to a multiple of 4."""
    _check("tissue_plane: image", image_u8, torch.uint8)
    if image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise ValueError(f"tissue_plane: image must be RGB [H,W,3] uint8 (got {tuple(image_u8.shape)})")
    H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
    pitch = -(-W // 4) * 4
    plane = torch.empty(H, pitch, dtype=torch.uint8, device=image_u8.device)
    K.call("selunet_tissue_plane", K.ptr(image_u8), H, W, int(bright), int(spread), K.ptr(plane), pitch, K.stream_ptr())
    return plane[:, :W]


def tile_tissue_counts(plane: torch.Tensor, origins: torch.Tensor, th: int, tw: int, flip: int = 0,
                       out: torch.Tensor | None = None) -> torch.Tensor:
    """`selunet_tile_tissue_counts`: plane uint8 [H,W] (tissue_plane's view, or any with contiguous rows) and
    origins int32 [n,2] -> int32 [n] (into `out` when given), the tissue pixels of each tile's th x tw window of
    the plane flipped by `flip` and continued by reflection: what `tile_gather_flip` would gather."""
    pitch = _plane("tile_tissue_counts", "plane", plane, torch.uint8)
    _check("tile_tissue_counts: origins", origins, torch.int32)
    if origins.dim() != 2 or origins.shape[1] != 2:
        raise ValueError(f"tile_tissue_counts: origins must be [n,2] (got {tuple(origins.shape)})")
    n = origins.shape[0]
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=plane.device)
    _check("tile_tissue_counts: out", out, torch.int32)
    if tuple(out.shape) != (n,):
        raise ValueError(f"tile_tissue_counts: out must be [{n}] (got {tuple(out.shape)})")
    out.zero_()  # the kernel adds
    K.call("selunet_tile_tissue_counts", K.ptr(plane), pitch, plane.shape[0], plane.shape[1], K.ptr(origins), n, th, tw,
           int(flip), K.ptr(out), K.stream_ptr())
    return out


def tissue_class_counts(mask: torch.Tensor, plane: torch.Tensor, counts: torch.Tensor | None = None) -> torch.Tensor:
    """`selunet_tissue_class_counts`: int64 [4] on the device, {background, tumor, abstained, pixels} of the
    0 / 255 / 127 mask [H,W] over the tissue pixels of plane [H,W] (added into `counts` when given)."""
    mp = _plane("tissue_class_counts", "mask", mask, torch.uint8)
    pp = _plane("tissue_class_counts", "plane", plane, torch.uint8, int(mask.shape[0]), int(mask.shape[1]))
    if counts is None:
        counts = torch.zeros(4, dtype=torch.int64, device=mask.device)  # uint64 bits
    _check("tissue_class_counts: counts", counts, torch.int64)
    if counts.numel() != 4:
        raise ValueError("tissue_class_counts: counts must hold 4 words")
    K.call("selunet_tissue_class_counts", K.ptr(mask), mp, K.ptr(plane), pp, mask.shape[0], mask.shape[1], K.ptr(counts),
           K.stream_ptr())
    return counts


# ----------------------------------------------------------------------------- regions
REGION_COLUMNS = ("label", "area", "y_min", "x_min", "y_max", "x_max", "sum_y", "sum_x", "prob_sum",
                  "abstain_contacts")
REGION_PIXELS_MAX = 2 ** 31 - 1  # labels are int32: 1 + y W + x
CLEANUP_NAMES = ("removed_regions", "removed_pixels", "filled_holes", "filled_pixels")
_REGION_PASSES = ((1, "local"), (2, "seam"), (4, "flatten"))
_TABLE_MIN_INIT = 2 ** 62


@dataclass
class Regions:
    """The region table: one int64 tensor [n] per column of REGION_COLUMNS, rows ascending by label. prob_sum
    is None when no prob8 plane was given. Every value is an exact integer; the centroid is
    (sum_y / area, sum_x / area) and the mean probability prob_sum / (255 area), formed on the host."""
    label: torch.Tensor
    area: torch.Tensor
    y_min: torch.Tensor
    x_min: torch.Tensor
    y_max: torch.Tensor
    x_max: torch.Tensor
    sum_y: torch.Tensor
    sum_x: torch.Tensor
    prob_sum: torch.Tensor | None
    abstain_contacts: torch.Tensor

    def __len__(self) -> int:
        return int(self.label.numel())

    def columns(self) -> tuple:
        return tuple(c for c in REGION_COLUMNS if getattr(self, c) is not None)

    def numpy(self) -> dict:
        """{column: int64 numpy [n]} in one transfer."""
        cols = self.columns()
        host = torch.stack([getattr(self, c) for c in cols]).cpu().numpy().astype(np.int64)
        return {c: host[i] for i, c in enumerate(cols)}

    def rows(self) -> list:
        """One dict of Python ints per region."""
        host = self.numpy()
        return [{c: int(v[i]) for c, v in host.items()} for i in range(len(self))]


def _region_args(fn, min_region, fill_holes, connectivity):
    if connectivity not in (4, 8):
        raise ValueError(f"{fn}: connectivity {connectivity!r}: 4 or 8")
    for name, v in (("min_region", min_region), ("fill_holes", fill_holes)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 0:
            raise ValueError(f"{fn}: {name} must be an integer >= 0 (got {v!r})")


def _region_size(fn, H, W):
    if H < 1 or W < 1 or H * W >= REGION_PIXELS_MAX:
        raise ValueError(f"{fn}: region labels need 1 <= H * W < 2^31 - 1 (got {H} x {W})")


def _plane(fn, name, t, dtype, H=None, W=None):
    """A 2-d cuda view whose rows are contiguous; returns its row pitch in elements."""
    if (not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != dtype or t.dim() != 2
            or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
        raise ValueError(f"{fn}: {name} must be a cuda {dtype} [H,W] tensor or a view of one with contiguous rows")
    if H is not None and tuple(t.shape) != (H, W):
        raise ValueError(f"{fn}: {name} must be [{H},{W}] like the mask (got {tuple(t.shape)})")
    return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])


class _Labelling:
    """One labelling: labels int32 [H,lp] (lp = W rounded up to 4), the positions and labels of the roots in
    ascending order, the plane holding each root's row at the root's position, and the device error word."""

    def __init__(self, H, W, lp, labels, rowidx, rp, label_col, err):
        self.H, self.W, self.lp, self.labels, self.rowidx, self.rp = H, W, lp, labels, rowidx, rp
        self.label_col, self.err = label_col, err

    @property
    def n(self) -> int:
        return int(self.label_col.numel())


def _raise_region_error(word: int):
    if word:
        names = ", ".join(n for b, n in _REGION_PASSES if word & b)
        raise K.SelunetError(f"selunet_regions_label: the {names} pass reached its iteration cap (error word {word}): "
                             "the label plane was corrupted while it ran")


def _label(fn, mask, value, connectivity) -> _Labelling:
    pitch = _plane(fn, "mask", mask, torch.uint8)
    H, W = int(mask.shape[0]), int(mask.shape[1])
    _region_size(fn, H, W)
    if not 0 <= int(value) <= 255:
        raise ValueError(f"{fn}: value must be in [0, 255] (got {value!r})")
    lp = -(-W // 4) * 4
    dev = mask.device
    with torch.cuda.device(dev):
        parent = torch.empty(H, lp, dtype=torch.int32, device=dev)  # uint32 bits
        labels = torch.empty(H, lp, dtype=torch.int32, device=dev)
        roots = torch.empty(H, lp, dtype=torch.uint8, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        K.call("selunet_regions_label", K.ptr(mask), pitch, H, W, int(value), int(connectivity), K.ptr(parent),
               K.ptr(labels), K.ptr(roots), lp, K.ptr(err), 7, K.stream_ptr())
        # the roots into ascending rows, once per labelling: raster order is label order. The parent plane
        # is done with; it becomes the root-indexed plane of row numbers.
        pos = torch.nonzero(roots.view(-1)).view(-1)
        parent.view(-1)[pos] = torch.arange(pos.numel(), dtype=torch.int32, device=dev)
        label_col = 1 + torch.div(pos, lp, rounding_mode="floor") * W + pos % lp
    return _Labelling(H, W, lp, labels, parent, lp, label_col, err)


def label_regions(mask: torch.Tensor, value: int = 255, connectivity: int = 8):
    """`selunet_regions_label`: the regions of `value` of a cuda uint8 [H,W] mask (possibly a view of a canvas)
    under connectivity 4 or 8. Returns (labels, n_regions): int32 [H,W], a view of a plane with padded rows,
    holding 1 + y W + x of the first pixel of each pixel's region (0 where the mask is not `value`)."""
    _region_args("label_regions", 0, 0, connectivity)
    lab = _label("label_regions", mask, value, connectivity)
    _raise_region_error(int(lab.err.item()))
    labels = lab.labels[:, :lab.W]
    labels._selunet_labelling = lab  # region_table finds the roots here instead of searching the plane again
    return labels, lab.n


def _labelling_of(fn, labels, H, W) -> _Labelling:
    lab = getattr(labels, "_selunet_labelling", None)
    if lab is not None and (lab.H, lab.W) == (H, W) and labels.data_ptr() == lab.labels.data_ptr():
        return lab
    # any int32 label plane in canonical form: its roots are the pixels that hold their own index
    lp = _plane(fn, "labels", labels, torch.int32, H, W)
    dev = labels.device
    own = (1 + torch.arange(H, dtype=torch.int32, device=dev)[:, None] * W
           + torch.arange(W, dtype=torch.int32, device=dev)[None, :])
    pos = torch.nonzero((labels == own).reshape(-1)).view(-1)
    rowidx = torch.empty(H, W, dtype=torch.int32, device=dev)
    rowidx.view(-1)[pos] = torch.arange(pos.numel(), dtype=torch.int32, device=dev)
    return _Labelling(H, W, lp, labels, rowidx, W, pos + 1, None)


def _table(fn, mask, lab: _Labelling, prob8) -> Regions:
    pitch = _plane(fn, "mask", mask, torch.uint8, lab.H, lab.W)
    ppitch = 0 if prob8 is None else _plane(fn, "prob8", prob8, torch.uint8, lab.H, lab.W)
    n, dev = lab.n, mask.device
    with torch.cuda.device(dev):
        table = torch.zeros(9, n, dtype=torch.int64, device=dev)  # uint64 bits
        table[1:3] = _TABLE_MIN_INIT
        if n:
            K.call("selunet_regions_stats", K.ptr(lab.labels), lab.lp, K.ptr(mask), pitch, K.ptr(prob8), ppitch, lab.H,
                   lab.W, K.ptr(lab.rowidx), lab.rp, n, K.ptr(table), K.stream_ptr())
    return Regions(lab.label_col, table[0], table[1], table[2], table[3], table[4], table[5], table[6],
                   None if prob8 is None else table[7], table[8])


def region_table(mask: torch.Tensor, labels: torch.Tensor, prob8: torch.Tensor | None = None) -> Regions:
    """`selunet_regions_stats`: the table of the regions that `labels` (label_regions' result, or any int32
    [H,W] plane in its form) marks in `mask`; prob8 (uint8 [H,W]) adds the column prob_sum."""
    _plane("region_table", "mask", mask, torch.uint8)
    H, W = int(mask.shape[0]), int(mask.shape[1])
    _region_size("region_table", H, W)
    if not torch.is_tensor(labels) or tuple(labels.shape) != (H, W):
        raise ValueError(f"region_table: labels must be [{H},{W}] like the mask")
    return _table("region_table", mask, _labelling_of("region_table", labels, H, W), prob8)


def _apply(fn, mask, lab, action, counts):
    pitch = _plane(fn, "mask", mask, torch.uint8)
    H, W = int(mask.shape[0]), int(mask.shape[1])
    with torch.cuda.device(mask.device):
        if lab is None:
            K.call("selunet_regions_apply", K.ptr(mask), pitch, H, W, None, 0, None, 0, None, 0, K.ptr(counts),
                   K.stream_ptr())
        else:
            _check(f"{fn}: action", action, torch.uint8)
            K.call("selunet_regions_apply", K.ptr(mask), pitch, H, W, K.ptr(lab.labels), lab.lp, K.ptr(lab.rowidx),
                   lab.rp, K.ptr(action), lab.n, K.ptr(counts), K.stream_ptr())


def clean_mask(mask: torch.Tensor, prob8: torch.Tensor | None = None, min_region: int = 0, fill_holes: int = 0,
               connectivity: int = 8):
    """The clean-up of DESIGN.md §7h on a 0 / 127 / 255 mask, in place: (1) min_region = N > 0: every region of
    255 under `connectivity` with area < N becomes 0; (2) fill_holes = M > 0: every region of 0 under the
    complementary connectivity whose bounding box touches no image border, that has no abstained 4-neighbour
    and whose area is <= M becomes 255. Returns (Regions of the 255-regions of the final mask, counts int64 [4]
    {background, tumor, abstained, pixels} of it, removed_regions, removed_pixels, filled_holes, filled_pixels);
    the scalars, the counts and the kernels' error word arrive in one read."""
    fn = "clean_mask"
    _region_args(fn, min_region, fill_holes, connectivity)
    _plane(fn, "mask", mask, torch.uint8)
    H, W = int(mask.shape[0]), int(mask.shape[1])
    _region_size(fn, H, W)
    if prob8 is not None:
        _plane(fn, "prob8", prob8, torch.uint8, H, W)
    dev = mask.device
    with torch.cuda.device(dev):
        scal = torch.zeros(9, dtype=torch.int64, device=dev)  # counts[4], CLEANUP_NAMES[4], error word
        spare = torch.zeros(4, dtype=torch.int64, device=dev)
        if min_region > 0:
            lab = _label(fn, mask, 255, connectivity)
            scal[8:9] |= lab.err
            if lab.n:
                reg = _table(fn, mask, lab, None)
                drop = reg.area < int(min_region)
                _apply(fn, mask, lab, drop.to(torch.uint8), spare)
                scal[4], scal[5] = drop.sum(), (reg.area * drop).sum()
        if fill_holes > 0:
            lab = _label(fn, mask, 0, 12 - connectivity)
            scal[8:9] |= lab.err
            if lab.n:
                reg = _table(fn, mask, lab, None)
                fill = ((reg.y_min > 0) & (reg.x_min > 0) & (reg.y_max < H - 1) & (reg.x_max < W - 1)
                        & (reg.abstain_contacts == 0) & (reg.area <= int(fill_holes)))
                _apply(fn, mask, lab, fill.to(torch.uint8) * 2, spare)
                scal[6], scal[7] = fill.sum(), (reg.area * fill).sum()
        lab = _label(fn, mask, 255, connectivity)
        scal[8:9] |= lab.err
        regions = _table(fn, mask, lab, prob8)
        _apply(fn, mask, None, None, scal)  # counts into scal[0:4]
        host = scal.cpu().numpy().astype(np.int64)  # the one read
    _raise_region_error(int(host[8]))
    return (regions, host[:4].copy()) + tuple(int(v) for v in host[4:8])


@dataclass
class Prediction:
    """`predict_image`'s result. logit, selection (None for a non-selective network), mask, prob8 (None when
    not asked for): device tensors [H,W], views of the canvases; counts: int64 numpy {background, tumor,
    abstained, pixels} over the image; plan: the tiling used. With test-time augmentation
    logit and selection are the means over `members` orientations, and votes / sel_votes (uint8 [H,W]) count
    the members with out >= t_out / sel >= t_sel; without it members is 1 and both are None (sel_votes also
    for a non-selective network)."""
    logit: torch.Tensor
    selection: torch.Tensor | None
    mask: torch.Tensor
    prob8: torch.Tensor | None
    counts: np.ndarray
    plan: TilePlan
    votes: torch.Tensor | None = None
    sel_votes: torch.Tensor | None = None
    members: int = 1
    regions: Regions | None = None  # with region analysis: the tumor regions of the final mask
    cleanup: dict | None = None     # and {removed_regions, removed_pixels, filled_holes, filled_pixels}
    # with tissue=True, else None: the tissue plane (uint8 [H,W] device view, 255 tissue / 0 glass),
    # `counts` over the tissue pixels only, per member a bool array over its plan's tiles (True: forwarded), and
    # the forwarded and all tiles summed over the members
    tissue: torch.Tensor | None = None
    tissue_counts: np.ndarray | None = None
    tiles_kept: list | None = None
    tiles_forwarded: int | None = None
    tiles_total: int | None = None
    # with stain=, else None: stain.normalize's info and the image that was predicted (uint8 [H,W,3] on
    # the device; the input itself where nothing could be fitted)
    stain: dict | None = None
    stain_image: torch.Tensor | None = None

    @property
    def unanimous_fraction(self) -> float | None:
        """The share of the image's pixels on which the members agree (votes 0 or all); None without votes."""
        if self.votes is None:
            return None
        v = self.votes
        return float(((v == 0) | (v == self.members)).sum().item()) / float(v.numel())

    @property
    def coverage(self) -> float:
        """The share of the image's pixels that were not abstained on."""
        return float(self.counts[0] + self.counts[1]) / float(self.counts[3])

    @property
    def tumor_fraction(self) -> float:
        """The share of tumor among the selected pixels (NaN when none is selected)."""
        sel = int(self.counts[0] + self.counts[1])
        return float(self.counts[1]) / sel if sel else float("nan")

    @property
    def tumor_fraction_of_tissue(self) -> float | None:
        """The share of tumor among the selected tissue pixels (NaN when there are none); None without tissue."""
        if self.tissue_counts is None:
            return None
        sel = int(self.tissue_counts[0] + self.tissue_counts[1])
        return float(self.tissue_counts[1]) / sel if sel else float("nan")


class _Skipped:
    """The output of a tile that is not forwarded: out = -inf and, with a selection head,
    sel = +inf, so that the existing stitch / accumulate write background, selected, prob8 0 and no tumor vote.
    One pair of constant buffers of up to `batch_size` tiles, made when the first tile is skipped."""

    def __init__(self, batch_size, tile, selective, device):
        self.shape, self.selective, self.device = (batch_size, tile, tile), selective, device
        self.out = self.sel = None

    def batches(self, origins_host, keep):
        """(out, sel, host origins, device origins) per batch of the tiles with keep False."""
        oh = np.ascontiguousarray(origins_host[~keep])
        if not len(oh):
            return
        if self.out is None:
            self.out = torch.full(self.shape, float("-inf"), dtype=torch.float32, device=self.device)
            self.sel = torch.full(self.shape, float("inf"), dtype=torch.float32, device=self.device) if self.selective else None
        od = torch.from_numpy(oh).to(self.device)
        for a in range(0, len(oh), self.shape[0]):
            b = min(a + self.shape[0], len(oh))
            yield self.out[:b - a], None if self.sel is None else self.sel[:b - a], oh[a:b], od[a:b]


def _kept_origins(origins_host, origins, keep):
    """The host and device origins of the tiles to forward: the plan's own when every tile is kept."""
    if keep is None or keep.all():
        return origins_host, origins
    oh = np.ascontiguousarray(origins_host[keep])
    return oh, torch.from_numpy(oh).to(origins.device)


def predict_image(net, image_u8, *, tile: int = 512, halo: int = HALO_MIN, batch_size: int = 16,
                  cut_off: float = 0.5, s_cut_off: float = 0.5, single_scale: str = "sigmoid",
                  input_type: str = "RGB", prob8: bool = True, allow_small_halo: bool = False,
                  tta: str = "none", regions: bool = False, min_region: int = 0, fill_holes: int = 0,
                  connectivity: int = 8, tissue: bool = False, tissue_bright: int = TISSUE_BRIGHT,
                  tissue_spread: int = TISSUE_SPREAD, tissue_min_pixels: int = 1, stain: ST.StainFit | None = None,
                  stain_beta: float = ST.BETA, _tissue_image: torch.Tensor | None = None) -> Prediction:
    """Apply `net` (a UNet_B on a cuda device, in eval mode) to `image_u8`, a numpy or torch uint8 [H,W,3] RGB
    image of any size: gather -> net -> stitch per batch of `batch_size` tiles, on the current stream.
    tta: "none", or "flips" / "d4": the mean over the 4 flips / the 8 flips and transposes of the image
    (`TTA_MEMBERS`), with the votes of the members.
    regions / min_region / fill_holes / connectivity: with `regions` or a clean-up size > 0 the
    mask is cleaned in place (`clean_mask`), counts are those of the cleaned mask, and `regions` / `cleanup`
    hold the table of its tumor regions and what the clean-up did; with the defaults nothing of that runs.
    tissue / tissue_bright / tissue_spread / tissue_min_pixels: with `tissue` a pixel is glass iff
    min(r,g,b) >= tissue_bright and max - min <= tissue_spread, and a tile whose input window holds fewer than
    tissue_min_pixels tissue pixels is not forwarded: its core is background, selected, logit -inf (selection
    +inf), prob8 0. The result gains tissue, tissue_counts, tiles_kept, tiles_forwarded and tiles_total; with the
    default nothing of that runs.
    stain / stain_beta: with a `StainFit` target the image is normalised to it on the device
    (`stain.normalize`) before it is tiled; gather, augmentation, stitch and regions run on the normalised image, the
    tissue plane is still the original's, and the result gains stain and stain_image. With None nothing of that runs."""
    if stain is not None:
        if not isinstance(stain, ST.StainFit):
            raise TypeError(f"predict_image: stain must be a stain.StainFit target or None (got {type(stain).__name__})")
        ST.beta_q_of(stain_beta)
        device = next(net.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("predict_image runs on the GPU only (no CPU fallback); move the network to a cuda device")
        img = image_u8 if torch.is_tensor(image_u8) else torch.from_numpy(np.ascontiguousarray(image_u8))
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError(f"predict_image: the image must be uint8 [H,W,3] RGB (got {img.dtype} {tuple(img.shape)})")
        with torch.cuda.device(device):
            img = img.to(device).contiguous()  # the one upload
            normalised, info = ST.normalize(img, stain, stain_beta)
        pred = predict_image(net, normalised, tile=tile, halo=halo, batch_size=batch_size, cut_off=cut_off,
                             s_cut_off=s_cut_off, single_scale=single_scale, input_type=input_type, prob8=prob8,
                             allow_small_halo=allow_small_halo, tta=tta, regions=regions, min_region=min_region,
                             fill_holes=fill_holes, connectivity=connectivity, tissue=tissue, tissue_bright=tissue_bright,
                             tissue_spread=tissue_spread, tissue_min_pixels=tissue_min_pixels,
                             _tissue_image=img if tissue else None)
        pred.stain, pred.stain_image = info, normalised
        return pred
    if tta not in TTA_MEMBERS:
        raise ValueError(f"predict_image: tta {tta!r}: one of {', '.join(map(repr, TTA_MEMBERS))}")
    _tissue_args("predict_image", tissue_bright, tissue_spread, tissue_min_pixels)
    rule = (int(tissue_bright), int(tissue_spread), int(tissue_min_pixels)) if tissue else None
    if net.training:
        raise RuntimeError("predict_image needs the network in eval mode (net.eval()): tiling is exact only with "
                           "the running BatchNorm statistics")
    if batch_size < 1:
        raise ValueError(f"predict_image: batch_size {batch_size} must be >= 1")
    device = next(net.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("predict_image runs on the GPU only (no CPU fallback); move the network to a cuda device")
    img = image_u8 if torch.is_tensor(image_u8) else torch.from_numpy(np.ascontiguousarray(image_u8))
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"predict_image: the image must be uint8 [H,W,3] RGB (got {img.dtype} {tuple(img.shape)})")
    H, W = int(img.shape[0]), int(img.shape[1])
    plan = TilePlan(H, W, tile, halo, allow_small_halo)
    _region_args("predict_image", min_region, fill_holes, connectivity)
    analyse = bool(regions) or min_region > 0 or fill_holes > 0
    if analyse:
        _region_size("predict_image", H, W)
        if regions and not prob8:
            raise ValueError("predict_image: regions=True reports prob_sum, which needs prob8=True")
    t_out = MT.logit_threshold("eval", cut_off, single_scale)
    t_sel = MT.logit_threshold("eval", s_cut_off, single_scale)
    selective = bool(net.selective)
    if analyse:
        pred = predict_image(net, img, tile=tile, halo=halo, batch_size=batch_size, cut_off=cut_off,
                             s_cut_off=s_cut_off, single_scale=single_scale, input_type=input_type, prob8=prob8,
                             allow_small_halo=allow_small_halo, tta=tta, tissue=tissue, tissue_bright=tissue_bright,
                             tissue_spread=tissue_spread, tissue_min_pixels=tissue_min_pixels, _tissue_image=_tissue_image)
        with torch.cuda.device(device):  # the stages read the mask and prob8 only: any forward path, any tta
            pred.regions, pred.counts, *done = clean_mask(pred.mask, pred.prob8, int(min_region), int(fill_holes),
                                                          connectivity)
            if rule:  # the tissue counts are those of the cleaned mask
                pred.tissue_counts = tissue_class_counts(pred.mask, pred.tissue).cpu().numpy().astype(np.int64)
        pred.cleanup = dict(zip(CLEANUP_NAMES, done))
        return pred
    if tta != "none":
        return _predict_tta(net, img, device, plan, TTA_MEMBERS[tta], batch_size, t_out, t_sel, input_type, prob8,
                            allow_small_halo, rule, _tissue_image)
    with torch.cuda.device(device), torch.no_grad():
        img = img.to(device).contiguous()  # the one upload
        origins = torch.from_numpy(plan.origins).to(device)
        keep = glass = None
        if rule:
            # of the original where the image was stain-normalised: the same tiles are forwarded
            glass = tissue_plane(img if _tissue_image is None else _tissue_image, rule[0], rule[1])
            # the one read before the first forward
            keep = tile_tissue_counts(glass, origins, tile, tile).cpu().numpy() >= rule[2]
        # the cores cover the canvases exactly once: no initial value is read
        logit = torch.empty(plan.Hc, plan.Wc, dtype=torch.float32, device=device)
        selection = torch.empty_like(logit) if selective else None
        mask = torch.empty(plan.Hc, plan.Wc, dtype=torch.uint8, device=device)
        prob = torch.empty_like(mask) if prob8 else None
        counts = torch.zeros(8 if rule else 4, dtype=torch.int64, device=device)  # uint64 bits
        image_counts = counts[:4] if rule else counts
        run_host, run = _kept_origins(plan.origins, origins, keep)  # the plan's own without a tissue rule
        n_run = len(run_host)
        x_buf = torch.empty(min(batch_size, plan.n), _CIN[input_type], tile, tile, dtype=torch.float32, device=device)
        for a in range(0, n_run, batch_size):
            b = min(a + batch_size, n_run)  # the last batch is run as ragged as it is
            x = tile_gather(img, run[a:b], tile, tile, input_type, out=x_buf[:b - a])
            res = net(x)
            out, sel = (res[0], res[1]) if selective else (res, None)
            tile_stitch(out.contiguous(), None if sel is None else sel.contiguous(), run_host[a:b], run[a:b],
                        halo, H, W, t_out, t_sel, logit, selection, mask, prob, image_counts)
        if rule:
            skipped = _Skipped(min(batch_size, plan.n), tile, selective, device)
            for out, sel, oh, od in skipped.batches(plan.origins, keep):
                tile_stitch(out, sel, oh, od, halo, H, W, t_out, t_sel, logit, selection, mask, prob, image_counts)
            tissue_class_counts(mask[:H, :W], glass, counts[4:])
        host_counts = counts.cpu().numpy().astype(np.int64)  # the one read
    pred = Prediction(logit[:H, :W], None if selection is None else selection[:H, :W], mask[:H, :W],
                      None if prob is None else prob[:H, :W], host_counts[:4], plan)
    if rule:
        pred.tissue, pred.tissue_counts, pred.tiles_kept = glass, host_counts[4:], [keep]
        pred.tiles_forwarded, pred.tiles_total = int(keep.sum()), plan.n
    return pred


def _predict_tta(net, img, device, plan, members, batch_size, t_out, t_sel, input_type, prob8, allow_small_halo,
                 rule=None, tissue_image=None):
    """predict_image with test-time augmentation. Member k = 4 c + f is the prediction of the
    image of orientation class c (0: the image; 1: its transpose, formed once on the device) flipped by f
    (bit 1 rows, bit 0 columns), mapped back. Per class, members run one after another: flipped gather -> net
    -> accumulate per batch of tiles into the class's fp32 sums and vote planes, whose rows are padded to a
    multiple of 8 pixels (zeros, never written); one finalize forms the mean and everything derived from it.
    rule = (bright, spread, min_pixels): every member skips the tiles of its own tiling whose
    window holds fewer than min_pixels tissue pixels; the window counts of all members are read at once before
    the first forward, and a skipped core is accumulated as -inf (selection +inf). tissue_image: the
    image the tissue planes are made of where `img` is its stain-normalised copy."""
    H, W, tile, halo = plan.H, plan.W, plan.tile, plan.halo
    selective = bool(net.selective)
    with torch.cuda.device(device), torch.no_grad():
        img = img.to(device).contiguous()  # the one upload
        x_buf = torch.empty(min(batch_size, plan.n), _CIN[input_type], tile, tile, dtype=torch.float32, device=device)
        oriented = {}

        def orientation(c):
            """(image, its plan, the plan's origins on the device) of class c, made when first asked for."""
            if c not in oriented:
                src = image_transpose(img) if c else img
                p = TilePlan(int(src.shape[0]), int(src.shape[1]), tile, halo, allow_small_halo) if c else plan
                oriented[c] = (src, p, torch.from_numpy(p.origins).to(device))  # the member's own tiling
            return oriented[c]

        kept = glass = None
        if rule:
            if tissue_image is None:
                glass = [tissue_plane(orientation(c)[0], rule[0], rule[1]) for c in range(members // 4)]  # per pixel
            else:
                glass = [tissue_plane(image_transpose(tissue_image) if c else tissue_image, rule[0], rule[1])
                         for c in range(members // 4)]
            sizes = [orientation(k // 4)[1].n for k in range(members)]
            window = torch.empty(sum(sizes), dtype=torch.int32, device=device)
            for k, part in enumerate(torch.split(window, sizes)):
                tile_tissue_counts(glass[k // 4], orientation(k // 4)[2], tile, tile, k & 3, out=part)
            host = window.cpu().numpy() >= rule[2]  # the one read before the first forward
            kept = np.split(host, np.cumsum(sizes)[:-1])
            skipped = _Skipped(min(batch_size, plan.n), tile, selective, device)
        classes = []
        for c in range(members // 4):
            src, p, origins = orientation(c)
            h, w = int(src.shape[0]), int(src.shape[1])
            ws = -(-w // 8) * 8
            sums = [torch.zeros(h, ws, dtype=torch.float32, device=device) if selective or i == 0 else None
                    for i in range(2)]
            vts = [torch.zeros(h, ws, dtype=torch.uint8, device=device) if selective or i == 0 else None
                   for i in range(2)]
            for f in range(4):
                keep = kept[4 * c + f] if rule else None
                run_host, run = _kept_origins(p.origins, origins, keep)  # the plan's own without a tissue rule
                for a in range(0, len(run_host), batch_size):
                    b = min(a + batch_size, len(run_host))
                    x = tile_gather_flip(src, run[a:b], tile, tile, input_type, f, out=x_buf[:b - a])
                    res = net(x)
                    out, sel = (res[0], res[1]) if selective else (res, None)
                    tta_accumulate(out.contiguous(), None if sel is None else sel.contiguous(), run_host[a:b],
                                   run[a:b], halo, f, f == 0, h, w, p.Hc, p.Wc, t_out, t_sel, sums[0], sums[1],
                                   vts[0], vts[1])
                if rule:
                    for out, sel, oh, od in skipped.batches(p.origins, keep):
                        tta_accumulate(out, sel, oh, od, halo, f, f == 0, h, w, p.Hc, p.Wc, t_out, t_sel, sums[0],
                                       sums[1], vts[0], vts[1])
            classes.append((sums[0], sums[1], vts[0], vts[1]))
        planes, counts = tta_finalize(classes[0], classes[1] if members == 8 else None, members, H, W, t_out, t_sel,
                                      prob8)
        if rule:
            counts = torch.cat([counts, tissue_class_counts(planes[2][:, :W], glass[0])])
        host_counts = counts.cpu().numpy().astype(np.int64)  # the one read
    logit, selection, mask, prob, votes, sel_votes = [None if t is None else t[:, :W] for t in planes]
    pred = Prediction(logit, selection, mask, prob, host_counts[:4], plan, votes, sel_votes, members)
    if rule:
        pred.tissue, pred.tissue_counts, pred.tiles_kept = glass[0], host_counts[4:], kept
        pred.tiles_forwarded, pred.tiles_total = int(sum(k.sum() for k in kept)), int(sum(sizes))
    return pred


# ----------------------------------------------------------------------------- CLI
def parse_arguments(argv=None):
    parser = argparse.ArgumentParser(description="whole-image prediction with a trained UNet_B")
    parser.add_argument('--input', type=str, nargs='+', required=True, help='image files or directories of images')
    parser.add_argument('--model_dir', type=str, required=True, help='directory holding exactly one .pth checkpoint')
    # ---- as eval's
    parser.add_argument('--model_arch', type=str, default='UNet_B', choices=['UNet_B'])
    parser.add_argument('--selective', type=bool, default=False, help='Is the network based on SelectiveNet?')
    parser.add_argument('--input_type', type=str, default='RGB')
    parser.add_argument('--cut_off', type=float, default=0.5, help='prob > cut_off -> pred: 1')
    parser.add_argument('--s_cut_off', type=float, default=0.5, help='selection > cut_off -> select: 1')
    parser.add_argument('--single_scale', type=str, default='sigmoid', choices=['None', 'clip', 'sigmoid', 'minmax'])
    parser.add_argument('--batch_size', type=int, default=16, help='tiles per forward')
    parser.add_argument('--local_rank', type=int, nargs='+', default=[0], help='local gpu ids (the first is used)')
    parser.add_argument('--save_dir', type=str, default='./output', help='saving results')
    parser.add_argument('--compute_dtype', type=str, default='fp32', choices=['fp32', 'bf16'])
    parser.add_argument('--fp32_path', type=str, default='exact', choices=['exact', 'split'],
                        help='conv kernels of the fp32 forward: exact fp32, or the split-fp16 kernels of training')
    # ---- tiling
    parser.add_argument('--tile', type=int, default=TILE_MAX, help='tile side, a multiple of 8, at most 512')
    parser.add_argument('--halo', type=int, default=HALO_MIN, help='halo, a multiple of 8, at least 56')
    parser.add_argument('--tta', type=str, default='none', choices=list(TTA_MEMBERS),
                        help='test-time augmentation: the mean over the 4 flips, or the 8 flips and transposes')
    # ---- region analysis and clean-up of the mask
    parser.add_argument('--regions', type=int, default=0, choices=[0, 1],
                        help='1: write <stem>_regions.csv, the table of the tumor regions')
    parser.add_argument('--min_region', type=int, default=0, help='remove tumor regions of fewer pixels (0: off)')
    parser.add_argument('--fill_holes', type=int, default=0,
                        help='fill background holes of at most this many pixels inside tumor (0: off)')
    parser.add_argument('--connectivity', type=int, default=8, choices=[4, 8],
                        help='connectivity of tumor regions; holes use the complementary one')
    # ---- tissue mask: glass tiles are not forwarded
    parser.add_argument('--tissue', type=int, default=0, choices=[0, 1],
                        help='1: skip tiles without tissue, write <stem>_tissue.png and the tissue counts')
    parser.add_argument('--tissue_bright', type=int, default=TISSUE_BRIGHT,
                        help='a pixel is glass iff min(r,g,b) >= this and max - min <= --tissue_spread')
    parser.add_argument('--tissue_spread', type=int, default=TISSUE_SPREAD, help='see --tissue_bright')
    parser.add_argument('--tissue_min_pixels', type=int, default=1,
                        help='a tile is forwarded iff its input window holds at least this many tissue pixels')
    # ---- stain normalisation of the image before it is tiled
    parser.add_argument('--stain_norm', type=str, default='none', choices=['none', 'macenko'],
                        help='macenko: fit the image and re-render it with the stains of --stain_target, write <stem>_stain.png')
    parser.add_argument('--stain_target', type=str, default=None,
                        help='the target, a JSON file made by `python -m ...stain fit` from training images '
                             '(default: the published Macenko reference)')
    parser.add_argument('--stain_beta', type=float, default=ST.BETA,
                        help='a pixel is fitted to iff each of its optical densities is at least this')
    args = parser.parse_args(argv)
    if args.stain_target is not None and args.stain_norm == 'none':
        parser.error('--stain_target needs --stain_norm macenko')
    if not 0.0 < args.stain_beta < 5.5:
        parser.error('--stain_beta must be in (0, 5.5), an optical density')
    if args.fp32_path == 'split' and args.compute_dtype == 'bf16':
        parser.error('--fp32_path split is an fp32 path: not with --compute_dtype bf16')
    if args.min_region < 0 or args.fill_holes < 0:
        parser.error('--min_region and --fill_holes must be >= 0')
    if not (0 <= args.tissue_bright <= 255 and 0 <= args.tissue_spread <= 255):
        parser.error('--tissue_bright and --tissue_spread must be in [0, 255]')
    if args.tissue_min_pixels < 1:
        parser.error('--tissue_min_pixels must be >= 1')
    return args


def list_inputs(inputs) -> list:
    """The image files named by --input, directories expanded (sorted, by extension); every stem once."""
    files = []
    for p in inputs:
        if os.path.isdir(p):
            found = sorted(f for f in os.listdir(p) if f.lower().endswith(IMAGE_EXTENSIONS))
            if not found:
                raise FileNotFoundError(f"no image files in {p}")
            files += [os.path.join(p, f) for f in found]
        elif os.path.isfile(p):
            files.append(p)
        else:
            raise FileNotFoundError(f"--input {p}: no such file or directory")
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    twice = sorted({s for s in stems if stems.count(s) > 1})
    if twice:
        raise ValueError(f"inputs share the stems {twice}: their outputs would overwrite each other")
    return files


def find_checkpoint(model_dir) -> str:
    names = sorted(c for c in os.listdir(model_dir) if c.endswith('.pth'))
    if not names:
        raise FileNotFoundError(f"no .pth checkpoint in {model_dir}")
    if len(names) > 1:
        raise ValueError(f"{model_dir} holds {len(names)} checkpoints ({', '.join(names)}): predict applies one "
                         "network; ensembles are eval's business")
    return os.path.join(model_dir, names[0])


def image_record(path, pred: Prediction) -> dict:
    """One image's entry of predict.json."""
    c = [int(v) for v in pred.counts]
    sel = c[0] + c[1]
    rec = {"input": path, "height": pred.plan.H, "width": pred.plan.W, "tile": pred.plan.tile,
           "halo": pred.plan.halo, "grid": list(pred.plan.grid), "tiles": pred.plan.n,
           "counts": dict(zip(COUNT_NAMES, c)),
           "tumor_fraction_of_selected": c[1] / sel if sel else None,
           "coverage": sel / c[3], "unanimous_fraction": pred.unanimous_fraction}
    if pred.regions is not None:  # only with region analysis: a plain run's file is what it was
        rec["regions"] = len(pred.regions)
        rec["largest_region_area"] = int(pred.regions.area.max().item()) if len(pred.regions) else 0
        rec["cleanup"] = {k: int(v) for k, v in pred.cleanup.items()}
    if pred.tissue_counts is not None:  # only with the tissue mask
        tc = [int(v) for v in pred.tissue_counts]
        rec["tissue_pixels"] = tc[3]
        rec["tissue_counts"] = dict(zip(COUNT_NAMES, tc))
        rec["tumor_fraction_of_tissue"] = tc[1] / (tc[0] + tc[1]) if tc[0] + tc[1] else None
        rec["tiles_forwarded"], rec["tiles_total"] = int(pred.tiles_forwarded), int(pred.tiles_total)
    if pred.stain is not None:  # only with stain normalisation
        rec["stain"] = dict(pred.stain)
    return rec


def region_csv_rows(regions: Regions) -> list:
    """The lines of <stem>_regions.csv: a header, then per region the table's columns and centroid_y = sum_y / area,
    centroid_x = sum_x / area, mean_prob = prob_sum / (255 area) (when prob_sum is there), each the correctly
    rounded quotient of the two integers, written by repr."""
    cols = regions.columns()
    derived = ("centroid_y", "centroid_x") + (("mean_prob",) if "prob_sum" in cols else ())
    lines = [",".join(cols + derived)]
    for r in regions.rows():
        vals = [str(r[c]) for c in cols] + [repr(r["sum_y"] / r["area"]), repr(r["sum_x"] / r["area"])]
        if "prob_sum" in cols:
            vals.append(repr(r["prob_sum"] / (255 * r["area"])))
        lines.append(",".join(vals))
    return lines


def write_regions_csv(path, regions: Regions):
    with open(path, "w") as fh:
        fh.write("\n".join(region_csv_rows(regions)) + "\n")


def predict_files(args) -> dict:
    from PIL import Image

    import selectivenet_for_semantic_segmentation_binary_amd as S
    from . import net_utils

    if args.input_type not in _MODE:
        raise ValueError(f"input_type {args.input_type!r}: 'RGB', 'GH' or 'H_RGB' (utils/data_utils.py:223-226)")
    files = list_inputs(args.input)
    ckpt = find_checkpoint(args.model_dir)
    TilePlan(8, 8, args.tile, args.halo)  # the tiling arguments, before anything is loaded
    target = None
    if args.stain_norm == 'macenko':
        target = ST.MACENKO_TARGET if args.stain_target is None else ST.load_target(args.stain_target)
    device = torch.device("cuda", args.local_rank[0])
    torch.cuda.set_device(device)
    dt = torch.bfloat16 if args.compute_dtype == 'bf16' else torch.float32
    net = S.UNet_B(args.input_type, selective=args.selective, compute_dtype=dt, fp32_eval_path=args.fp32_path)
    net_utils.net_test_load(ckpt, net)
    net = net.to(device).train(False)
    os.makedirs(args.save_dir, exist_ok=True)
    doc = {"checkpoint": ckpt, "selective": bool(args.selective), "input_type": args.input_type,
           "cut_off": args.cut_off, "s_cut_off": args.s_cut_off, "single_scale": args.single_scale, "tta": args.tta,
           "images": []}
    if args.tissue:  # only with the tissue mask: a plain run's file is what it was
        doc.update(tissue_bright=args.tissue_bright, tissue_spread=args.tissue_spread,
                   tissue_min_pixels=args.tissue_min_pixels)
        doc["images"] = doc.pop("images")  # the list stays last
    if target is not None:  # only with stain normalisation
        doc.update(stain_norm=args.stain_norm, stain_target=target.to_json(), stain_beta=args.stain_beta)
        doc["images"] = doc.pop("images")
    for path in files:
        image = np.array(Image.open(path).convert("RGB"))
        pred = predict_image(net, image, tile=args.tile, halo=args.halo, batch_size=args.batch_size,
                             cut_off=args.cut_off, s_cut_off=args.s_cut_off, single_scale=args.single_scale,
                             input_type=args.input_type, tta=args.tta, regions=bool(args.regions),
                             min_region=args.min_region, fill_holes=args.fill_holes, connectivity=args.connectivity,
                             tissue=bool(args.tissue), tissue_bright=args.tissue_bright,
                             tissue_spread=args.tissue_spread, tissue_min_pixels=args.tissue_min_pixels, stain=target,
                             stain_beta=args.stain_beta)
        stem = os.path.join(args.save_dir, os.path.splitext(os.path.basename(path))[0])
        mask = pred.mask.cpu().numpy()
        Image.fromarray(mask).save(stem + "_mask.png")
        Image.fromarray(pred.prob8.cpu().numpy()).save(stem + "_prob.png")
        if args.selective:
            Image.fromarray(np.where(mask != 127, 255, 0).astype(np.uint8)).save(stem + "_select.png")
        if pred.votes is not None:
            votes = pred.votes.cpu().numpy().astype(np.int64)
            Image.fromarray((votes * 255 // pred.members).astype(np.uint8)).save(stem + "_votes.png")
        if pred.regions is not None:
            write_regions_csv(stem + "_regions.csv", pred.regions)
        if pred.tissue is not None:
            Image.fromarray(pred.tissue.cpu().numpy()).save(stem + "_tissue.png")
        if pred.stain_image is not None:
            Image.fromarray(pred.stain_image.cpu().numpy()).save(stem + "_stain.png")
        rec = image_record(path, pred)
        doc["images"].append(rec)
        c = rec["counts"]
        print(f'    {path}: {rec["height"]} x {rec["width"]}, {rec["grid"][0]} x {rec["grid"][1]} tiles, tumor '
              f'{c["tumor"]} background {c["background"]} abstained {c["abstained"]} (coverage {rec["coverage"]:.4f})')
    with open(os.path.join(args.save_dir, "predict.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    return doc


def main(argv=None):
    args = parse_arguments(sys.argv[1:] if argv is None else argv)
    print('\nargs={}\n'.format(args))
    predict_files(args)
    return 0


if __name__ == '__main__':
    sys.exit(main())
