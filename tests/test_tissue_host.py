"""The tissue mask of whole-image prediction without a GPU: the pixel rule and the window counts
of tests/_tissue_ref.py on the fixed half-glass image (pinned skip counts of every ensemble member), the glass
model under the default rule, and the refusals of `predict_image`, the CLI and the three entry points
(host-side, before any launch)."""
import numpy as np
import pytest

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import build as B
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR
from tests import _predict_ref as R
from tests import _tissue_ref as T
from tests import _tta_ref as TR


# ----------------------------------------------------------------------------- the rule and the fixed image
@pytest.fixture(scope="module")
def image():
    return T.fixed_image()


def test_defaults_are_the_glass_model_at_six_standard_deviations():
    assert PR.TISSUE_BRIGHT == T.BRIGHT == int(np.floor(255 * (0.96 - 6 * 0.005))) == 237
    assert PR.TISSUE_SPREAD == T.SPREAD == int(np.ceil(255 * 6 * np.sqrt(2) * 0.005)) == 11


def test_pixel_rule_at_its_edges():
    px = np.array([[(237, 237, 237), (236, 240, 240), (237, 248, 240), (237, 249, 240), (255, 255, 255), (0, 0, 0)]], np.uint8)
    assert T.plane_of(px).tolist() == [[0, 255, 0, 255, 0, 255]]
    assert T.plane_of(px, 0, 255).tolist() == [[0] * 6]        # everything is glass
    assert T.plane_of(px, 255, 0).tolist() == [[255] * 4 + [0, 255]]  # only saturated white is
    assert T.plane_of(px, 0, 0).tolist() == [[0, 255, 255, 255, 0, 0]]  # every grey is


def test_fixed_image_is_half_tissue_half_glass(image):
    assert image.shape == (200, 296, 3) and image.dtype == np.uint8
    plane = T.plane_of(image)
    assert (plane[:, :148] == 255).all()
    ys, xs = np.nonzero(plane[:, 148:])
    assert ys.tolist() == [10] and (xs + 148).tolist() == [250]  # all glass but the speck
    assert PR.TilePlan(200, 296, T.TILE, T.HALO).n == 35 and PR.TilePlan(296, 200, T.TILE, T.HALO).n == 35


def test_window_counts_count_reflected_copies_again():
    plane = np.zeros((1, 9), np.uint8)
    plane[0, 2] = 255
    # columns -8 .. 15 of a width-9 row fold onto 8..1, 0..8, 7..1: column 2 is met three times, every row the same
    assert T.window_counts(plane, [(-8, -8)], 24, 24).tolist() == [3 * 24]
    assert T.window_counts(plane, [(-8, -8)], 24, 24, flip=1).tolist() == [3 * 24]  # column 6 of the flipped row
    plane[0, 0] = 255
    assert T.window_counts(plane, [(0, 0)], 8, 8).tolist() == [2 * 8]
    assert T.window_counts(plane, [(0, 0)], 8, 8, flip=1).tolist() == [1 * 8]  # of columns 8 and 6 of the flipped row, 6
    assert T.window_counts(np.full((37, 53), 255, np.uint8), [(-8, -8), (30, 40)], 24, 40, flip=2).tolist() == [960, 960]


@pytest.mark.parametrize("min_pixels,skipped", [(1, 6), (3, 8), (5, 10)])
def test_pinned_skip_counts_of_the_plain_plan(image, min_pixels, skipped):
    kept = T.kept_of(image, 0, min_pixels)
    assert kept.shape == (35,) and int((~kept).sum()) == skipped


def test_pinned_skip_counts_of_every_member(image):
    skipped = [int((~T.kept_of(image, k)).sum()) for k in range(8)]
    assert skipped == [6, 3, 4, 2, 6, 4, 3, 2]  # every member both keeps and skips tiles
    # with the default, a skipped tile's whole window is glass: so is its core
    plane = T.plane_of(image)
    for k in range(8):
        src = np.ascontiguousarray(TR.T(k, plane))
        cover = T.core_cover(src.shape, T.kept_of(image, k))
        assert not src[~cover].any() and (~cover).any(), k


def test_a_million_samples_of_the_glass_model_are_glass():
    sample = T.glass((1000, 1000, 3), 11)
    assert 238 <= int(sample.min()) and int(sample.max()) <= 252 and len(np.unique(sample)) > 8
    assert not T.plane_of(sample).any()


# ----------------------------------------------------------------------------- predict_image and the CLI
class _Net:  # refused before the network is looked at
    training = False


@pytest.mark.parametrize("kw,word", [
    (dict(tissue_bright=256), "tissue_bright"), (dict(tissue_bright=-1), "tissue_bright"),
    (dict(tissue_bright=237.0), "tissue_bright"), (dict(tissue_spread=256), "tissue_spread"),
    (dict(tissue_spread=-1), "tissue_spread"), (dict(tissue_min_pixels=0), "tissue_min_pixels"),
    (dict(tissue_min_pixels=-3), "tissue_min_pixels"), (dict(tissue_min_pixels=1.5), "tissue_min_pixels"),
    (dict(tissue_min_pixels=True), "tissue_min_pixels")])
@pytest.mark.parametrize("tissue", [False, True])
def test_predict_image_refuses_bad_tissue_arguments(kw, word, tissue):
    with pytest.raises(ValueError, match=word):
        PR.predict_image(_Net(), np.zeros((8, 8, 3), np.uint8), tissue=tissue, **kw)


BASE = ["--input", "x.png", "--model_dir", "ck"]


def test_cli_defaults_and_flags():
    a = PR.parse_arguments(BASE)
    assert (a.tissue, a.tissue_bright, a.tissue_spread, a.tissue_min_pixels) == (0, 237, 11, 1)
    a = PR.parse_arguments(BASE + ["--tissue", "1", "--tissue_bright", "0", "--tissue_spread", "255", "--tissue_min_pixels", "64"])
    assert (a.tissue, a.tissue_bright, a.tissue_spread, a.tissue_min_pixels) == (1, 0, 255, 64)


@pytest.mark.parametrize("flags", [["--tissue", "2"], ["--tissue_bright", "256"], ["--tissue_bright", "-1"],
                                   ["--tissue_spread", "256"], ["--tissue_spread", "-1"], ["--tissue_min_pixels", "0"],
                                   ["--tissue_min_pixels", "-1"], ["--tissue_bright", "237.5"]])
def test_cli_refuses_out_of_range_tissue_flags(flags, capsys):
    with pytest.raises(SystemExit) as e:
        PR.parse_arguments(BASE + flags)
    assert e.value.code == 2 and "--tissue" in capsys.readouterr().err


def test_record_has_no_tissue_keys_without_tissue():
    plan = PR.TilePlan(8, 8, 160, 56)
    pred = PR.Prediction(None, None, None, None, np.array([40, 20, 4, 64]), plan)
    assert pred.tissue is None and pred.tissue_counts is None and pred.tiles_kept is None
    assert pred.tiles_forwarded is None and pred.tiles_total is None and pred.tumor_fraction_of_tissue is None
    assert list(PR.image_record("x.png", pred)) == ["input", "height", "width", "tile", "halo", "grid", "tiles", "counts",
                                                    "tumor_fraction_of_selected", "coverage", "unanimous_fraction"]
    pred.tissue_counts, pred.tiles_forwarded, pred.tiles_total = np.array([30, 10, 2, 42]), 1, 1
    rec = PR.image_record("x.png", pred)
    assert rec["tissue_pixels"] == 42 and rec["tissue_counts"] == dict(zip(PR.COUNT_NAMES, [30, 10, 2, 42]))
    assert rec["tumor_fraction_of_tissue"] == pred.tumor_fraction_of_tissue == 0.25
    assert (rec["tiles_forwarded"], rec["tiles_total"]) == (1, 1)
    pred.tissue_counts = np.zeros(4, np.int64)
    assert np.isnan(pred.tumor_fraction_of_tissue) and PR.image_record("x.png", pred)["tumor_fraction_of_tissue"] is None


# ----------------------------------------------------------------------------- C ABI argument rules
@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(K.lib_path()):
        B.build()
    return K.load()


A = 0x10000  # a 16-B aligned address that is never dereferenced: every call below is refused on the host

ARGS = {
    "selunet_tissue_plane": dict(img=A, H=37, W=53, bright=237, spread=11, plane=A, pitch=56, stream=None),
    "selunet_tile_tissue_counts": dict(plane=A, pitch=56, H=37, W=53, origins=A, n=3, th=24, tw=40, flip=3, counts=A,
                                       stream=None),
    "selunet_tissue_class_counts": dict(mask=A, mask_pitch=56, plane=A, pitch=56, H=37, W=53, counts=A, stream=None),
}
# (call, the arguments that differ from ARGS, a word of the message)
REFUSALS = [
    ("selunet_tissue_plane", dict(img=None), "null"), ("selunet_tissue_plane", dict(plane=None), "null"),
    ("selunet_tissue_plane", dict(H=0), "height and width"), ("selunet_tissue_plane", dict(W=65536), "height and width"),
    ("selunet_tissue_plane", dict(bright=256), "[0, 255]"), ("selunet_tissue_plane", dict(bright=-1), "[0, 255]"),
    ("selunet_tissue_plane", dict(spread=256), "[0, 255]"), ("selunet_tissue_plane", dict(spread=-1), "[0, 255]"),
    ("selunet_tissue_plane", dict(pitch=52), "row pitch"), ("selunet_tissue_plane", dict(pitch=54), "row pitch"),
    ("selunet_tissue_plane", dict(pitch=53), "row pitch"), ("selunet_tissue_plane", dict(plane=A + 2), "4-B aligned"),
    ("selunet_tile_tissue_counts", dict(plane=None), "null"), ("selunet_tile_tissue_counts", dict(counts=None), "null"),
    ("selunet_tile_tissue_counts", dict(origins=None), "null origins"), ("selunet_tile_tissue_counts", dict(n=0), "n must"),
    ("selunet_tile_tissue_counts", dict(H=0), "height and width"), ("selunet_tile_tissue_counts", dict(W=65536), "height and width"),
    ("selunet_tile_tissue_counts", dict(th=20), "multiples of 8"), ("selunet_tile_tissue_counts", dict(tw=4), "multiples of 8"),
    ("selunet_tile_tissue_counts", dict(pitch=52), "row pitch"), ("selunet_tile_tissue_counts", dict(flip=4), "flip"),
    ("selunet_tile_tissue_counts", dict(flip=-1), "flip"), ("selunet_tile_tissue_counts", dict(th=65536, tw=32768), "32-bit"),
    ("selunet_tile_tissue_counts", dict(counts=A + 2), "4-B aligned"),
    ("selunet_tissue_class_counts", dict(mask=None), "null"), ("selunet_tissue_class_counts", dict(plane=None), "null"),
    ("selunet_tissue_class_counts", dict(counts=None), "null"), ("selunet_tissue_class_counts", dict(H=0), "height and width"),
    ("selunet_tissue_class_counts", dict(W=65536), "height and width"), ("selunet_tissue_class_counts", dict(mask_pitch=52), "row pitches"),
    ("selunet_tissue_class_counts", dict(pitch=52), "row pitches"), ("selunet_tissue_class_counts", dict(counts=A + 4), "8-B aligned"),
]


@pytest.mark.parametrize("fn,bad,word", REFUSALS, ids=[f"{f[8:]}:{','.join(f'{k}={v}' for k, v in b.items())}"[:60]
                                                       for f, b, _ in REFUSALS])
def test_tissue_calls_refuse_on_the_host(lib, fn, bad, word):
    args = dict(ARGS[fn])
    args.update(bad)
    assert lib is not None and getattr(lib, fn)(*args.values()) == 1
    assert fn[len("selunet_"):].encode() in lib.selunet_last_error() and word.encode() in lib.selunet_last_error()
    with pytest.raises(K.SelunetError, match=fn[len("selunet_"):]):
        K.call(fn, *args.values())


def test_bindings_match_the_argument_counts(lib):
    for fn, args in ARGS.items():
        assert len(K.SIGNATURES[fn][1]) == len(args), fn
    assert {f for f, _, _ in REFUSALS} == set(ARGS)
    assert R.refl(-1, 9) == 1  # the fold the window counts rest on
