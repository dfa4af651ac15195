"""Region analysis without a GPU: the numpy reference (tests/_regions_ref.py) against
scipy.ndimage.label and against hand-checked tables, the argument rules of the three entry points and of the
Python wrappers, and the CLI's parser and writers on a fabricated Prediction."""
import csv
import io
import json
import os

import numpy as np
import pytest
import torch

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import build as B
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR
from tests import _regions_ref as RR

PATTERNS = {
    "zeros": lambda H, W: np.zeros((H, W), np.uint8),
    "full": lambda H, W: np.full((H, W), 255, np.uint8),
    "checkerboard": RR.checkerboard,
    "diagonals": lambda H, W: RR.diagonals(H, W, 8),
    "spiral": RR.spiral,
    "serpentine": RR.serpentine,
    "comb": RR.comb,
    "noise41": lambda H, W: RR.noise(H, W, 0.41, 1),
    "noise59": lambda H, W: RR.noise(H, W, 0.59, 2),
    "blobs": lambda H, W: RR.blobs(H, W, 3),
}


# ----------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_reference_labels_equal_scipy_after_relabelling(name, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    for H, W in ((1, 9), (9, 1), (37, 53)):
        mask = PATTERNS[name](H, W)
        got = RR.label(mask, 255, connectivity)
        structure = np.ones((3, 3), int) if connectivity == 8 else None
        theirs, n = ndimage.label(mask == 255, structure=structure)
        # canonical form of scipy's labelling: every region named by its first pixel in raster order
        first = np.full(n + 1, H * W, np.int64)
        np.minimum.at(first, theirs.ravel(), np.arange(H * W))
        want = np.where(theirs > 0, 1 + first[theirs], 0)
        assert np.array_equal(got, want), (name, H, W)
        assert len(np.unique(got[got > 0])) == n
        assert got.dtype == np.int32 and ((got > 0) == (mask == 255)).all()


def test_reference_patterns_are_what_they_are_meant_to_be():
    H, W = 20, 31
    assert len(np.unique(RR.label(RR.checkerboard(H, W), 255, 8))) == 2  # 0 and one region
    assert (RR.label(RR.checkerboard(H, W), 255, 4) > 0).sum() == len(np.unique(RR.label(RR.checkerboard(H, W), 255, 4))) - 1
    for pattern in (RR.serpentine, RR.spiral, RR.comb):
        m = pattern(H, W)
        lab = RR.label(m, 255, 4)
        assert set(np.unique(lab)) == {0, 1} and (m == 255).sum() > H * W // 3, pattern.__name__
    assert set(np.unique(RR.blobs(H, W, 3))) == {0, 127, 255}
    # both diagonal directions pass through the corners of the 8 x 8 tiles
    d = RR.diagonals(24, 24, 8)
    assert d[7, 7] == d[8, 8] == 255 and d[7, 8] == d[8, 7] == 255


def rows_of(t):
    return [dict(zip(t, (int(v[i]) for v in t.values()))) for i in range(len(t["label"]))]


def test_hand_checked_table():
    m = np.array([[255, 255, 0, 0, 255],
                  [0, 255, 0, 127, 255],
                  [0, 0, 255, 0, 0],
                  [255, 0, 0, 0, 127]], np.uint8)
    p = np.arange(20, dtype=np.uint8).reshape(4, 5) * 10
    # 8: (0,0),(0,1),(1,1),(2,2) form one region; (0,4),(1,4) a second; (3,0) a third
    t8 = rows_of(RR.table(m, RR.label(m, 255, 8), p))
    assert t8 == [
        dict(label=1, area=4, y_min=0, x_min=0, y_max=2, x_max=2, sum_y=3, sum_x=4, prob_sum=0 + 10 + 60 + 120,
             abstain_contacts=0),
        dict(label=5, area=2, y_min=0, x_min=4, y_max=1, x_max=4, sum_y=1, sum_x=8, prob_sum=40 + 90, abstain_contacts=1),
        dict(label=16, area=1, y_min=3, x_min=0, y_max=3, x_max=0, sum_y=3, sum_x=0, prob_sum=150, abstain_contacts=0)]
    # 4: the pixel (2,2) is a region of its own, named 1 + 2 * 5 + 2
    t4 = RR.table(m, RR.label(m, 255, 4))
    assert t4["label"].tolist() == [1, 5, 13, 16] and t4["area"].tolist() == [3, 2, 1, 1] and "prob_sum" not in t4
    # the regions of 0 under 4: contacts count ordered pairs, so a pixel with two abstained neighbours counts 2
    z = RR.table(m, RR.label(m, 0, 4))
    assert z["label"].tolist() == [3, 6] and z["area"].tolist() == [3, 8]
    # (0,3) and (1,2) see (1,3); (2,3) sees (1,3), (3,3) and (2,4) see (3,4)
    assert z["abstain_contacts"].tolist() == [2, 3]


def test_hole_rule_at_an_image_border():
    m = np.full((5, 6), 255, np.uint8)
    m[2, 2] = 0          # an inner hole
    m[0, 4] = 0          # a hole in the first row: its box touches the border
    m[3, 5] = 0          # and one in the last column
    out, t, counts, done = RR.clean(m, fill_holes=10)
    assert done == dict(removed_regions=0, removed_pixels=0, filled_holes=1, filled_pixels=1)
    assert out[2, 2] == 255 and out[0, 4] == 0 and out[3, 5] == 0
    assert counts == [2, 28, 0, 30] and t["area"].tolist() == [28]


def test_hole_touching_an_abstained_pixel_stays():
    m = np.full((7, 9), 255, np.uint8)
    m[2, 2:4] = 0        # a clean hole of two pixels
    m[4, 5] = 0          # a hole whose right neighbour abstains
    m[4, 6] = 127
    out, t, counts, done = RR.clean(m, fill_holes=2)
    assert done["filled_holes"] == 1 and done["filled_pixels"] == 2
    assert (out[2, 2:4] == 255).all() and out[4, 5] == 0 and out[4, 6] == 127
    assert RR.clean(m, fill_holes=1)[3]["filled_holes"] == 0  # area <= M: the two-pixel hole is too large for M = 1
    assert counts == [1, 61, 1, 63] and t["abstain_contacts"].tolist() == [3]  # (3,6), (5,6), (4,7) see (4,6)


def test_hole_with_a_diagonal_leak_under_4_and_8():
    m = np.zeros((7, 7), np.uint8)
    m[1:6, 1:6] = 255
    m[3, 3] = 0          # the hole
    m[2, 2] = 0          # a diagonal way from the hole ...
    m[1, 1] = 0          # ... to the outside
    # tumor 8-connected: holes are 4-connected, the diagonal does not leak, (3,3) and (2,2) are holes of one pixel
    out8, _, _, done8 = RR.clean(m, fill_holes=5, connectivity=8)
    assert done8["filled_holes"] == 2 and out8[3, 3] == 255 and out8[2, 2] == 255 and out8[1, 1] == 0
    # tumor 4-connected: holes are 8-connected, (3,3)-(2,2)-(1,1)-(0,0) is one region of 0 touching the border
    out4, _, _, done4 = RR.clean(m, fill_holes=5, connectivity=4)
    assert done4["filled_holes"] == 0 and np.array_equal(out4, m)


def test_min_region_threshold_is_strict_and_precedes_the_filling():
    m = np.zeros((6, 12), np.uint8)
    m[1, 1:4] = 255                   # area 3
    m[3:5, 1:3] = 255                 # area 4
    m[1:4, 6:9] = 255
    m[2, 7] = 0                       # a ring of 8 around a hole
    out, t, counts, done = RR.clean(m, min_region=4, fill_holes=1)
    assert done == dict(removed_regions=1, removed_pixels=3, filled_holes=1, filled_pixels=1)
    assert (out[1, 1:4] == 0).all() and (out[3:5, 1:3] == 255).all() and out[2, 7] == 255
    assert t["area"].tolist() == [9, 4] and counts == [72 - 13, 13, 0, 72]
    # a ring below min_region goes first, and then its hole is no hole any more
    out, t, counts, done = RR.clean(m, min_region=9, fill_holes=1)
    assert done == dict(removed_regions=3, removed_pixels=15, filled_holes=0, filled_pixels=0) and not out.any()


# ----------------------------------------------------------------------------- C ABI argument rules
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(K.lib_path()):
        B.build()
    return K.load()


A = 0x10000  # a 16-B aligned address that is never dereferenced: every call below is refused on the host


def call_args(names, defaults, **kw):
    a = dict(defaults)
    a.update(kw)
    return [a[k] for k in names]


LABEL = ("mask", "pitch", "H", "W", "value", "connectivity", "parent", "labels", "roots", "lp", "err", "passes", "stream")
LABEL_OK = dict(mask=A + 3, pitch=56, H=37, W=53, value=255, connectivity=8, parent=A, labels=A, roots=A, lp=56, err=A,
                passes=7, stream=None)
LABEL_BAD = [dict(mask=None), dict(parent=None), dict(labels=None), dict(roots=None), dict(err=None), dict(H=0), dict(W=0),
             dict(H=46341, W=46341, lp=46344, pitch=46341), dict(pitch=52), dict(value=-1), dict(value=256),
             dict(connectivity=6), dict(connectivity=0), dict(lp=53), dict(lp=60), dict(lp=52), dict(parent=A + 4),
             dict(labels=A + 8), dict(roots=A + 2), dict(err=A + 2), dict(H=2 ** 31 - 2, W=1, lp=4, pitch=1),
             dict(passes=0), dict(passes=8)]
STATS = ("labels", "lp", "mask", "pitch", "prob8", "ppitch", "H", "W", "rowidx", "rp", "n_rows", "table", "stream")
STATS_OK = dict(labels=A, lp=56, mask=A + 1, pitch=53, prob8=A + 1, ppitch=53, H=37, W=53, rowidx=A, rp=56, n_rows=5,
                table=A, stream=None)
STATS_BAD = [dict(labels=None), dict(mask=None), dict(rowidx=None), dict(table=None), dict(H=0), dict(W=-1), dict(lp=52),
             dict(rp=52), dict(pitch=52), dict(ppitch=52), dict(n_rows=0), dict(n_rows=37 * 53 + 1), dict(labels=A + 2),
             dict(rowidx=A + 2), dict(table=A + 4), dict(H=65536, W=32768)]
APPLY = ("mask", "pitch", "H", "W", "labels", "lp", "rowidx", "rp", "action", "n_rows", "counts", "stream")
APPLY_OK = dict(mask=A + 1, pitch=53, H=37, W=53, labels=A, lp=56, rowidx=A, rp=56, action=A + 1, n_rows=5, counts=A,
                stream=None)
APPLY_BAD = [dict(mask=None), dict(counts=None), dict(labels=None), dict(rowidx=None), dict(action=None),
             dict(labels=None, rowidx=None), dict(H=0), dict(W=0), dict(pitch=52), dict(lp=52), dict(rp=52),
             dict(n_rows=0), dict(n_rows=37 * 53 + 1), dict(labels=A + 2), dict(rowidx=A + 2), dict(counts=A + 4)]
CASES = ([("selunet_regions_label", LABEL, LABEL_OK, b) for b in LABEL_BAD]
         + [("selunet_regions_stats", STATS, STATS_OK, b) for b in STATS_BAD]
         + [("selunet_regions_apply", APPLY, APPLY_OK, b) for b in APPLY_BAD])


@pytest.mark.parametrize("fn,names,ok,bad", CASES,
                         ids=[f"{c[0][16:]}:" + ",".join(f"{k}={v}" for k, v in c[3].items()) for c in CASES])
def test_region_calls_refuse_on_the_host(lib, fn, names, ok, bad):
    assert getattr(lib, fn)(*call_args(names, ok, **bad)) == 1
    assert fn[len("selunet_"):].encode() in lib.selunet_last_error()
    with pytest.raises(K.SelunetError, match=fn[len("selunet_"):]):
        K.call(fn, *call_args(names, ok, **bad))


def test_region_bindings_match_the_argument_counts():
    for fn, names in (("selunet_regions_label", LABEL), ("selunet_regions_stats", STATS), ("selunet_regions_apply", APPLY)):
        assert len(K.SIGNATURES[fn][1]) == len(names), fn


# ----------------------------------------------------------------------------- Python argument rules
class _Net:
    """As much of a network on a cuda device as predict_image asks for before it refuses."""
    training, selective = False, True

    def parameters(self):
        class P:
            device = torch.device("cuda", 0)
        yield P()


@pytest.mark.parametrize("kw,word", [
    (dict(min_region=-1), "min_region"), (dict(fill_holes=-5), "fill_holes"), (dict(min_region=1.5), "min_region"),
    (dict(regions=True, connectivity=6), "connectivity"), (dict(connectivity=0), "connectivity"),
    (dict(regions=True, prob8=False), "prob8")])
def test_predict_image_refuses_region_arguments_before_anything_runs(kw, word):
    with pytest.raises(ValueError, match=word):
        PR.predict_image(_Net(),np.zeros((16, 16, 3), np.uint8), tile=160, halo=56, **kw)


def test_wrappers_refuse_bad_arguments():
    cpu = torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="connectivity"):
        PR.label_regions(cpu, 255, 5)
    with pytest.raises(ValueError, match="cuda"):
        PR.label_regions(cpu)
    with pytest.raises(ValueError, match="fill_holes"):
        PR.clean_mask(cpu, fill_holes=-1)
    with pytest.raises(ValueError, match="cuda"):
        PR.clean_mask(cpu, min_region=3)
    with pytest.raises(ValueError, match=r"2\^31"):
        PR._region_size("label_regions", 46341, 46341)
    PR._region_size("label_regions", 46340, 46341)
    PR.TilePlan(65535, 65535)  # the plain limit stays


# ----------------------------------------------------------------------------- CLI
BASE = ["--input", "x.png", "--model_dir", "m"]


def test_cli_region_flags():
    a = PR.parse_arguments(BASE)
    assert (a.regions, a.min_region, a.fill_holes, a.connectivity) == (0, 0, 0, 8)
    a = PR.parse_arguments(BASE + "--regions 1 --min_region 40 --fill_holes 9 --connectivity 4".split())
    assert (a.regions, a.min_region, a.fill_holes, a.connectivity) == (1, 40, 9, 4)
    for bad in ("--connectivity 6", "--min_region -1", "--fill_holes -2", "--regions 2", "--min_region x"):
        with pytest.raises(SystemExit):
            PR.parse_arguments(BASE + bad.split())


def fabricated(with_regions):
    plan = PR.TilePlan(100, 140, 160, 56)
    z = torch.zeros(100, 140, dtype=torch.uint8)
    pred = PR.Prediction(z.float(), None, z, z, np.array([13000, 900, 100, 14000], np.int64), plan)
    if with_regions:
        t = lambda *v: torch.tensor(v, dtype=torch.int64)  # noqa: E731
        pred.regions = PR.Regions(label=t(5, 1401), area=t(3, 897), y_min=t(0, 10), x_min=t(4, 0), y_max=t(0, 60),
                                  x_max=t(6, 139), sum_y=t(0, 31000), sum_x=t(15, 62001), prob_sum=t(700, 200001),
                                  abstain_contacts=t(0, 17))
        pred.cleanup = dict(removed_regions=4, removed_pixels=9, filled_holes=1, filled_pixels=2)
    return pred


def test_record_has_no_new_keys_without_the_feature():
    plain = PR.image_record("a.png", fabricated(False))
    assert list(plain) == ["input", "height", "width", "tile", "halo", "grid", "tiles", "counts",
                           "tumor_fraction_of_selected", "coverage", "unanimous_fraction"]
    assert fabricated(False).regions is None and fabricated(False).cleanup is None
    rec = PR.image_record("a.png", fabricated(True))
    assert list(rec)[:len(plain)] == list(plain) and {k: rec[k] for k in plain} == plain
    assert rec["regions"] == 2 and rec["largest_region_area"] == 897
    assert rec["cleanup"] == dict(removed_regions=4, removed_pixels=9, filled_holes=1, filled_pixels=2)
    json.dumps(rec)
    empty = fabricated(True)
    empty.regions = PR.Regions(*[torch.zeros(0, dtype=torch.int64)] * 10)
    assert PR.image_record("a.png", empty)["largest_region_area"] == 0 and PR.image_record("a.png", empty)["regions"] == 0


def test_regions_csv(tmp_path):
    reg = fabricated(True).regions
    PR.write_regions_csv(tmp_path / "a_regions.csv", reg)
    text = (tmp_path / "a_regions.csv").read_text()
    got = list(csv.reader(io.StringIO(text)))
    assert got[0] == list(PR.REGION_COLUMNS) + ["centroid_y", "centroid_x", "mean_prob"] and len(got) == 3
    assert got[1] == ["5", "3", "0", "4", "0", "6", "0", "15", "700", "0", repr(0 / 3), repr(15 / 3), repr(700 / (255 * 3))]
    assert got[2][-3:] == [repr(31000 / 897), repr(62001 / 897), repr(200001 / (255 * 897))]
    assert float(got[2][-3]) == 31000 / 897  # repr round-trips: the quotient is on disk exactly
    assert reg.rows()[1]["x_max"] == 139 and reg.numpy()["area"].tolist() == [3, 897] and len(reg) == 2
    # without prob8: neither prob_sum nor mean_prob
    reg.prob_sum = None
    lines = PR.region_csv_rows(reg)
    assert "prob" not in lines[0] and lines[0].endswith("abstain_contacts,centroid_y,centroid_x") and len(lines) == 3
