"""Host side of tests/test_gpu_first_layer_loops.py, test_gpu_io_loops.py and test_gpu_regions_tiles.py (no GPU): the
launchers' grid rules and caps as those modules assume them, restated from csrc/, and every size they use held in
the regime it claims. A launcher whose rule changes fails here first, before a GPU test silently returns to one
tile or one pass per workgroup. Also the labels the many-tile region tests take as known, against the flood fill."""
import numpy as np
import pytest

from tests import _regions_ref as RR
from tests import test_gpu_first_layer_loops as FL
from tests import test_gpu_io_loops as IO
from tests import test_gpu_regions_tiles as RT


def cdiv(a, b):
    return -(-a // b)


# csrc/first_layer.hip: selunet_first_conv_fwd_centered, wgrad_tiles_per_block / first_wgrad_launch
def fwd_plan(n, h, w):
    tiles = n * cdiv(h, 16) * cdiv(w, 16)
    grid = min(tiles, 3072)
    return tiles, grid, [len(range(b, tiles, grid)) for b in (0, grid - 1)]  # tiles of the first and last workgroup


def wgrad_plan(n, h, w):
    tiles = n * cdiv(h, 16) * cdiv(w, 16)
    per = max(1, cdiv(tiles, 1024))
    rows = cdiv(tiles, per)
    return tiles, per, rows, tiles - (rows - 1) * per


def test_first_layer_forward_regimes():
    assert (FL.FWD_WGS, FL.WGRAD_WGS, FL.FT) == (3072, 1024, 16)
    tiles, grid, (first, last) = fwd_plan(*FL.F1[2:])
    assert tiles == 6150 > 2 * 3072 and grid == 3072 and (first, last) == (3, 2)  # workgroups with 3 and with 2 tiles
    n, h, w = FL.F1[2:]
    per_image = cdiv(h, 16) * cdiv(w, 16)
    assert per_image == 6 and 3072 % per_image == 0 and cdiv(h, 16) == 3  # an interior tile row; the tiles of one
    assert (0 // per_image) != (3072 // per_image)                        # workgroup lie in different images
    assert w % 16 == 1 and h % 16 == 1                                    # 1-pixel-wide and 1-pixel-high edge tiles
    tiles, grid, (first, last) = fwd_plan(*FL.F2[2:])
    assert tiles == 3078 and grid == 3072 and (first, last) == (2, 1) and tiles - grid == 6
    for case in FL.EDGE:
        tiles, grid, per_wg = fwd_plan(*case[2:])
        assert tiles == grid and per_wg[0] == 1
    assert {c[1] for c in FL.EDGE} == {1, 2, 3}


def test_first_layer_wgrad_regimes():
    assert wgrad_plan(*FL.W1[2:]) == (2056, 3, 686, 1)
    assert wgrad_plan(*FL.W2[2:]) == (1029, 2, 515, 1)
    n, h, w = FL.W1[2:]
    assert (cdiv(h, 16) * cdiv(w, 16)) % 3 != 0  # 4 tiles per image, 3 per block: blocks span two images
    for case in FL.EDGE:
        tiles, per, rows, last = wgrad_plan(*case[2:])
        assert per == 1 and rows == tiles
    mask, own = FL.last_block_mask(2, 17, 31, 3)  # 8 tiles, blocks of 3: the last holds tiles 6 and 7 of image 1
    assert own == 2 and not mask[0].any() and mask[1, 0, 16:, :].all() and not mask[1, 0, :16, :].any()


# The grid-stride launches (csrc/train_io.hip, predict_io.hip, predict_tta.hip, predict_tissue.hip,
# predict_regions.hip, boundary.hip): grid = io_grid(cdiv(items, 256), cap); rows kernels: cdiv(items, 1024), 64 in x
CAPS = {"prep_batch": 8192, "seg_metrics": 2048, "tile_gather": 8192, "tile_stitch": 2048, "tile_gather_flip": 8192,
        "tta_accumulate": 8192, "tissue_plane": 8192, "tissue_class_counts": 2048, "regions_flatten": 16384,
        "regions_apply": 16384, "boundary_bands": 2048}
ROW_CAPS = {"seg_metrics_rows": 64, "boundary_rows": 64}


def passes(items, grid):
    return cdiv(items, grid * 256)


@pytest.mark.parametrize("name", list(CAPS) + list(ROW_CAPS))
def test_io_sizes_wrap_under_the_small_grids(name):
    items = IO.ITEMS[name]
    IO.wraps(items)
    own = cdiv(items, 1024) if name in ROW_CAPS else cdiv(items, 256)
    cap = ROW_CAPS.get(name) or CAPS[name]
    assert own <= cap  # uncapped today: the default grid makes one pass (the rows kernels four)
    for g in (3, 1):
        grid = max(1, min(own, g))
        assert passes(items, grid) >= 4 and items % (grid * 256)  # >= 3 full passes and a ragged last one


def test_region_tile_counts_and_loops():
    assert [(cdiv(h, 64), cdiv(w, 64)) for h, w in RT.SIZES] == [(16, 16), (16, 18)]
    for h, w in RT.SIZES:
        ty, tx = cdiv(h, 64), cdiv(w, 64)
        seam = (ty - 1) * w + (tx - 1) * h
        flatten = h * cdiv(w, 4)
        assert cdiv(seam, 256) <= 16384 and cdiv(flatten, 256) <= 16384  # one pass at the default grid
        assert passes(seam, 3) >= 4 and passes(flatten, 3) >= 4          # many under IO_GRID = 3
    assert RT.GRIDS == (-1, 3)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ["spiral", "serpentine", "comb", "checkerboard"])
def test_analytic_labels_equal_the_flood_fill(name, connectivity):
    mask = RT.PATTERNS[name](70, 130)
    assert np.array_equal(RR.analytic_labels(name, mask, connectivity), RR.label(mask, 255, connectivity))


def test_canonical_renames_to_the_first_raster_index():
    mask = RR.blobs(70, 130, 5)
    want = RR.label(mask, 255, 8)
    names = np.unique(want)
    shuffled = np.random.Generator(np.random.PCG64(1)).permutation(len(names) - 1) + 1
    other = np.concatenate([[0], shuffled])[np.searchsorted(names, want)]  # the same regions under other names
    assert np.array_equal(RR.canonical(other), want)


def test_tile_sums_follow_the_raster_order_of_tiles():
    import torch

    n, h, w = 2, 17, 31
    v = torch.arange(n * h * w, dtype=torch.float64).reshape(n, h, w, 1)
    got = FL.tile_sums(v, n, h, w)
    assert got.shape == (8, 1)
    assert got[3, 0] == v[0, 16:, 16:].sum() and got[4, 0] == v[1, :16, :16].sum()  # (image, tile row, tile column)
