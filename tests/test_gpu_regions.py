"""Region analysis on the GPU: labels, every column of the region table, the cleaned masks and
the counts against tests/_regions_ref.py, bit for bit (everything is an exact integer: there is nothing to
tolerate); then `predict_image(..., regions=, min_region=, fill_holes=)` and the predict CLI's files."""
import csv
import functools
import json

import numpy as np
import pytest
import torch

import selectivenet_for_semantic_segmentation_binary_amd as S
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR
from tests import _predict_ref as R
from tests import _regions_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the local tile is 64 x 64: sizes below, at and above one tile and two tiles in either direction, beside the
# fixed ones; (200, 300) has 4 x 5 tiles, so seams that meet seams
SHAPES = [(1, 1), (1, 9), (9, 1), (37, 53), (64, 64), (65, 129), (33, 130), (200, 300), (63, 65), (128, 127), (129, 64)]
PATTERNS = {
    "zeros": lambda H, W: np.zeros((H, W), np.uint8),
    "full": lambda H, W: np.full((H, W), 255, np.uint8),
    "corners": lambda H, W: corners(H, W),
    "checkerboard": RR.checkerboard,
    "diagonals": RR.diagonals,   # through the corners of the 64 x 64 tiles, both directions
    "spiral": RR.spiral,
    "serpentine": RR.serpentine,
    "comb": RR.comb,
    "noise41": lambda H, W: RR.noise(H, W, 0.41, 41),
    "noise59": lambda H, W: RR.noise(H, W, 0.59, 59),
}


def corners(H, W):
    m = np.zeros((H, W), np.uint8)
    m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = 255
    return m


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


@functools.lru_cache(maxsize=None)
def pattern(name, H, W):
    m = PATTERNS[name](H, W)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def prob_plane(H, W):
    p = np.random.Generator(np.random.PCG64(H * 1000 + W)).integers(0, 256, (H, W), dtype=np.uint8)
    p.setflags(write=False)
    return p


def table_of(reg):
    return {k: v.tolist() for k, v in reg.numpy().items()}


def check_labelling(mask, value, connectivity, prob8=None, mask_dev=None):
    """label_regions and region_table of `mask` against the reference, every bit; returns the device labels."""
    H, W = mask.shape
    want = RR.label(mask, value, connectivity)
    want_table = {k: v.tolist() for k, v in RR.table(mask, want, prob8).items()}
    m = dev(mask) if mask_dev is None else mask_dev
    labels, n = PR.label_regions(m, value, connectivity)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (H, W)
    got = labels.cpu().numpy()
    assert np.array_equal(got, want), f"labels differ at {int((got != want).sum())} of {H * W} pixels"
    assert n == len(want_table["label"])
    p = None if prob8 is None else dev(prob8)
    reg = PR.region_table(m, labels, p)
    assert table_of(reg) == want_table and len(reg) == n
    assert list(table_of(reg)) == [c for c in PR.REGION_COLUMNS if c != "prob_sum" or prob8 is not None]
    return labels, reg


# ----------------------------------------------------------------------------- labels and table
@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("name", list(PATTERNS))
def test_labels_and_table_equal_the_reference(name, H, W, connectivity):
    check_labelling(pattern(name, H, W), 255, connectivity, prob_plane(H, W))


def test_pattern_facts():
    """What the patterns are there for, on the reference: one region across every seam, or very many."""
    H, W = 200, 300
    assert len(np.unique(RR.label(pattern("checkerboard", H, W), 255, 8))) == 2
    assert len(np.unique(RR.label(pattern("checkerboard", H, W), 255, 4))) == H * W // 2 + 1
    for name in ("spiral", "serpentine", "comb"):
        lab = RR.label(pattern(name, H, W), 255, 4)
        assert set(np.unique(lab)) == {0, 1}, name  # a single 4-connected region that starts at (0, 0)
    d = pattern("diagonals", H, W)
    assert d[63, 63] == d[64, 64] == d[63, 64] == d[64, 63] == 255 and d[127, 128] == d[128, 127] == 255
    assert len(np.unique(RR.label(d, 255, 8))) < 12 < H < len(np.unique(RR.label(d, 255, 4)))  # joined by diagonal steps only


@pytest.mark.parametrize("H,W", [(37, 53), (65, 129), (200, 300)])
def test_three_valued_mask_labelled_at_255_and_at_0(H, W):
    mask = RR.blobs(H, W, H + W)
    assert set(np.unique(mask)) == {0, 127, 255}
    for value, connectivity in ((255, 8), (255, 4), (0, 4), (0, 8)):
        _, reg = check_labelling(mask, value, connectivity, prob_plane(H, W))
        assert int(reg.abstain_contacts.sum().item()) > 0
    # 127 itself can be labelled too
    check_labelling(mask, 127, 8)


def test_a_view_of_a_canvas_and_the_bytes_outside_it():
    H, W = 65, 129
    mask = RR.blobs(H, W, 7)
    for oy, ox, Hc, Wc in ((0, 0, 72, 136), (3, 5, 80, 150)):  # [:H, :W], and a view that starts at an odd address
        canvas = np.random.Generator(np.random.PCG64(oy)).choice(np.array([0, 127, 255], np.uint8), (Hc, Wc))
        canvas[oy:oy + H, ox:ox + W] = mask
        c = dev(canvas)
        view = c[oy:oy + H, ox:ox + W]
        assert view.stride(0) == Wc != W
        pc = dev(np.pad(prob_plane(H, W), ((oy, Hc - H - oy), (ox, Wc - W - ox))))
        pview = pc[oy:oy + H, ox:ox + W]
        for value, connectivity in ((255, 8), (0, 4)):
            want = RR.label(mask, value, connectivity)
            labels, n = PR.label_regions(view, value, connectivity)
            assert np.array_equal(labels.cpu().numpy(), want)
            reg = PR.region_table(view, labels, pview)
            assert table_of(reg) == {k: v.tolist() for k, v in RR.table(mask, want, prob_plane(H, W)).items()}
        assert np.array_equal(c.cpu().numpy(), canvas)  # labelling writes nothing
        want_mask, want_table, want_counts, done = RR.clean(mask, prob_plane(H, W), 6, 4, 8)
        assert done["removed_regions"] > 0 and done["filled_holes"] > 0
        reg, counts, *scalars = PR.clean_mask(view, pview, 6, 4, 8)
        after = c.cpu().numpy()
        assert np.array_equal(after[oy:oy + H, ox:ox + W], want_mask) and counts.tolist() == want_counts
        assert table_of(reg) == {k: v.tolist() for k, v in want_table.items()}
        assert scalars == [done[k] for k in PR.CLEANUP_NAMES]
        after[oy:oy + H, ox:ox + W] = canvas[oy:oy + H, ox:ox + W]
        assert np.array_equal(after, canvas)  # every byte outside the view is as it was


def test_two_calls_give_identical_bits_and_the_error_word_is_zero():
    H, W = 200, 300
    for name, connectivity in (("noise59", 4), ("noise41", 8), ("serpentine", 4), ("spiral", 8), ("comb", 4)):
        m, p = dev(pattern(name, H, W)), dev(prob_plane(H, W))
        runs = []
        for _ in range(2):
            lab = PR._label("test", m, 255, connectivity)
            assert int(lab.err.item()) == 0
            reg = PR._table("test", m, lab, p)
            runs.append((lab.labels.cpu().numpy().copy(), table_of(reg)))
        assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
        assert (runs[0][0][:, W:] == 0).all()  # the padding columns of the label plane hold no label


def test_region_table_of_a_label_plane_from_elsewhere():
    """labels that did not come from label_regions (a copy, here): the roots are found in the plane itself."""
    H, W = 65, 129
    mask = RR.blobs(H, W, 11)
    m = dev(mask)
    labels, n = PR.label_regions(m, 255, 8)
    want = {k: v.tolist() for k, v in RR.table(mask, RR.label(mask, 255, 8), prob_plane(H, W)).items()}
    assert table_of(PR.region_table(m, labels.clone(), dev(prob_plane(H, W)))) == want
    assert table_of(PR.region_table(m, dev(RR.label(mask, 255, 8)), dev(prob_plane(H, W)))) == want


# ----------------------------------------------------------------------------- clean-up
N_MIN, M_MAX = 7, 5


def cleanup_mask(H=70, W=140):
    """Regions of area exactly N - 1 and N; holes of area exactly M and M + 1 inside a slab that crosses the tile
    border at column 64; a hole at the image's border; a hole touching a 127; a diagonal leak."""
    m = np.zeros((H, W), np.uint8)
    m[2, 2:2 + N_MIN - 1] = 255          # area N - 1: goes
    m[5, 2:2 + N_MIN] = 255              # area N: stays
    m[8, 2:5] = m[9, 4:7] = 255          # area 6 = N - 1, joined under 8 only through (8,4)-(9,4): one region either way
    m[12, 2:5] = m[13, 5:8] = 255        # two regions of 3 under 4, one of 6 under 8: all go either way
    m[20:60, 40:120] = 255               # the slab
    m[25, 60:60 + M_MAX] = 0             # a hole of M across column 64: filled
    m[30, 60:60 + M_MAX + 1] = 0         # a hole of M + 1: stays
    m[35, 50] = 0                        # a hole next to an abstained pixel: stays
    m[35, 51] = 127
    m[40, 70] = m[41, 71] = 0            # two holes of 1 under 4; one hole of 2 under 8: filled either way
    m[22, 42] = m[21, 41] = m[20, 40] = 0  # a diagonal way to the outside: two holes of 1 under 4, no hole under 8
    m[59, 100] = 0                       # open to the outside under 4 and 8 (the slab's last row)
    m[0:4, 130:140] = 255                # a block in the image's corner ...
    m[0, 134] = m[2, 139] = 0            # ... with holes on the image's border: stay
    m[1, 132] = 0                        # and an inner one: filled
    m[45, 80] = 127                      # an abstained pixel inside the slab: never changed
    m.setflags(write=False)
    return m


CLEAN_MASKS = {"built": cleanup_mask, "blobs": lambda: RR.blobs(65, 129, 5), "noise": lambda: RR.noise(130, 70, 0.59, 9),
               "blobs_large": lambda: RR.blobs(200, 300, 6)}


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("min_region,fill_holes", [(N_MIN, 0), (0, M_MAX), (N_MIN, M_MAX), (0, 0), (10 ** 9, 0),
                                                   (0, 10 ** 9), (1, 1)])
@pytest.mark.parametrize("name", list(CLEAN_MASKS))
def test_clean_mask_equals_the_reference(name, min_region, fill_holes, connectivity):
    mask = CLEAN_MASKS[name]()
    H, W = mask.shape
    want_mask, want_table, want_counts, done = RR.clean(mask, prob_plane(H, W), min_region, fill_holes, connectivity)
    if name == "built" and (min_region, fill_holes) == (N_MIN, M_MAX):
        # the construction does what it is for, on the reference
        assert (want_mask[2, 2:8] == 0).all() and (want_mask[5, 2:9] == 255).all() and (want_mask[12:14, 2:8] == 0).all()
        assert (want_mask[25, 60:65] == 255).all() and (want_mask[30, 60:66] == 0).all() and want_mask[35, 50] == 0
        assert want_mask[59, 100] == 0 and want_mask[0, 134] == 0 and want_mask[2, 139] == 0 and want_mask[1, 132] == 255
        assert want_mask[40, 70] == want_mask[41, 71] == 255
        # tumor under 8: holes under 4, the diagonal does not leak; tumor under 4: holes under 8, it does
        assert (want_mask[22, 42] == 255) == (want_mask[21, 41] == 255) == (connectivity == 8) and want_mask[20, 40] == 0
        assert want_mask[45, 80] == 127 and want_mask[35, 51] == 127
    m = dev(mask)
    reg, counts, *scalars = PR.clean_mask(m, dev(prob_plane(H, W)), min_region, fill_holes, connectivity)
    got = m.cpu().numpy()
    assert np.array_equal(got, want_mask), f"{int((got != want_mask).sum())} pixels differ"
    assert counts.dtype == np.int64 and counts.tolist() == want_counts and int(counts[:3].sum()) == int(counts[3]) == H * W
    assert table_of(reg) == {k: v.tolist() for k, v in want_table.items()}
    assert scalars == [done[k] for k in PR.CLEANUP_NAMES]
    assert np.array_equal(got == 127, mask == 127)  # abstained pixels are never changed
    if (min_region, fill_holes) == (0, 0):
        assert np.array_equal(got, mask) and counts.tolist() == RR.counts(mask) and scalars == [0, 0, 0, 0]
    if min_region == 10 ** 9:
        assert not (got == 255).any() and len(reg) == 0 and table_of(reg)["area"] == []


def test_clean_mask_without_prob8_has_no_prob_sum():
    mask = cleanup_mask()
    m = dev(mask)
    reg, counts, *_ = PR.clean_mask(m, None, N_MIN, M_MAX)
    want_mask, want_table, want_counts, _ = RR.clean(mask, None, N_MIN, M_MAX)
    assert reg.prob_sum is None and "prob_sum" not in want_table
    assert table_of(reg) == {k: v.tolist() for k, v in want_table.items()} and counts.tolist() == want_counts


# ----------------------------------------------------------------------------- whole path
H_I, W_I = 100, 140
KW = dict(tile=160, halo=56)


def make_net(state, **kw):
    net = S.UNet_B("RGB", selective=True, **kw)
    net.load_state_dict(state)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def whole():
    """The calibrated network and the 100 x 140 image of tests/_predict_ref.py. As in tests/test_gpu_predict_tta.py
    the cut-offs are set from the planes themselves (sigmoid of each head's median), so that all three mask values
    occur; min_region and fill_holes are then read off the reference's table of the plain mask: one more than the
    smallest tumor region, and the smallest hole that qualifies after step 1."""
    state = R.state_dict_of(*R.calibrated_state())
    net = make_net(state)
    image = R.sample_image(H_I, W_I)
    first = PR.predict_image(net, image, batch_size=4, **KW)
    cuts = [float(1.0 / (1.0 + np.exp(-np.median(t.cpu().numpy().astype(np.float64)))))
            for t in (first.logit, first.selection)]
    kw = dict(KW, cut_off=cuts[0], s_cut_off=cuts[1])
    plain = PR.predict_image(net, image, batch_size=4, **kw)
    mask = plain.mask.cpu().numpy()
    assert min(plain.counts[:3]) > 0.02 * H_I * W_I
    sizes = choose_sizes(mask)
    return {"state": state, "net": net, "image": image, "kw": kw, "plain": plain, "mask": mask, **sizes}


def choose_sizes(mask):
    H, W = mask.shape
    t = RR.table(mask, RR.label(mask, 255, 8))
    min_region = int(t["area"].min()) + 1
    step1, _, _, _ = RR.clean(mask, None, min_region, 0, 8)
    z = RR.table(step1, RR.label(step1, 0, 4))
    ok = (z["y_min"] > 0) & (z["x_min"] > 0) & (z["y_max"] < H - 1) & (z["x_max"] < W - 1) & (z["abstain_contacts"] == 0)
    assert ok.any(), "the plain mask has no hole that qualifies"
    return {"min_region": min_region, "fill_holes": int(z["area"][ok].min())}


def check_prediction(pred, base_mask, prob8, w, connectivity=8):
    want_mask, want_table, want_counts, done = RR.clean(base_mask, prob8, w["min_region"], w["fill_holes"], connectivity)
    assert done["removed_regions"] >= 1 and done["filled_holes"] >= 1  # the case is not vacuous
    assert np.array_equal(pred.mask.cpu().numpy(), want_mask)
    assert pred.counts.tolist() == want_counts and int(pred.counts[3]) == H_I * W_I
    assert table_of(pred.regions) == {k: v.tolist() for k, v in want_table.items()}
    assert pred.cleanup == done
    return done


def test_predict_image_with_regions_equals_the_reference_on_the_plain_mask(whole):
    w = whole
    plain = w["plain"]
    pred = PR.predict_image(w["net"], w["image"], batch_size=4, regions=True, min_region=w["min_region"],
                            fill_holes=w["fill_holes"], **w["kw"])
    done = check_prediction(pred, w["mask"], plain.prob8.cpu().numpy(), w)
    print(f"whole path: min_region {w['min_region']}, fill_holes {w['fill_holes']}: {done}; {len(pred.regions)} regions, "
          f"counts {plain.counts.tolist()} -> {pred.counts.tolist()}")
    for k in ("logit", "selection", "prob8"):  # untouched
        assert torch.equal(getattr(pred, k), getattr(plain, k)), k
    assert pred.votes is None and pred.members == 1
    # the table alone: the mask stays, regions are those of the plain mask
    only = PR.predict_image(w["net"], w["image"], batch_size=4, regions=True, **w["kw"])
    assert torch.equal(only.mask, plain.mask) and only.counts.tolist() == plain.counts.tolist()
    assert only.cleanup == dict.fromkeys(PR.CLEANUP_NAMES, 0)
    assert table_of(only.regions) == {k: v.tolist() for k, v in
                                      RR.table(w["mask"], RR.label(w["mask"], 255, 8), plain.prob8.cpu().numpy()).items()}
    # clean-up without prob8: allowed when only the clean-up is asked for
    bare = PR.predict_image(w["net"], w["image"], batch_size=4, min_region=w["min_region"], prob8=False, **w["kw"])
    assert bare.prob8 is None and bare.regions.prob_sum is None and bare.cleanup["removed_regions"] >= 1


def test_predict_image_without_the_new_arguments_is_the_plain_path(whole):
    w = whole
    a = w["plain"]
    b = PR.predict_image(w["net"], w["image"], batch_size=4, regions=False, min_region=0, fill_holes=0, connectivity=4,
                         **w["kw"])
    assert a.regions is None and a.cleanup is None and b.regions is None and b.cleanup is None
    for k in ("logit", "selection", "mask", "prob8"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.counts.tolist() == b.counts.tolist()
    assert np.array_equal(a.mask.cpu().numpy(), w["mask"])  # the feature's runs in between left the plain result alone


def test_regions_with_tta_on_the_split_path_and_in_bf16(whole):
    w = whole
    sizes = dict(min_region=w["min_region"], fill_holes=w["fill_holes"])
    for net, tta in ((w["net"], "flips"), (make_net(w["state"], fp32_eval_path="split"), "none"),
                     (make_net(w["state"], compute_dtype=torch.bfloat16), "none")):
        base = PR.predict_image(net, w["image"], batch_size=4, tta=tta, **w["kw"])
        pred = PR.predict_image(net, w["image"], batch_size=4, tta=tta, regions=True, connectivity=4, **sizes, **w["kw"])
        want_mask, want_table, want_counts, done = RR.clean(base.mask.cpu().numpy(), base.prob8.cpu().numpy(),
                                                            connectivity=4, **sizes)
        assert np.array_equal(pred.mask.cpu().numpy(), want_mask) and pred.counts.tolist() == want_counts
        assert table_of(pred.regions) == {k: v.tolist() for k, v in want_table.items()} and pred.cleanup == done
        assert (pred.votes is None) == (tta == "none")
        if tta != "none":
            assert torch.equal(pred.votes, base.votes) and torch.equal(pred.logit, base.logit)


def test_regions_without_a_selection_head(whole):
    net = S.UNet_B("RGB", selective=False)
    net.load_state_dict({k: v for k, v in whole["state"].items() if k in net.state_dict()})
    net = net.to(DEV).eval()
    base = PR.predict_image(net, whole["image"], batch_size=4, **KW)
    pred = PR.predict_image(net, whole["image"], batch_size=4, regions=True, min_region=20, fill_holes=20, **KW)
    want_mask, want_table, want_counts, done = RR.clean(base.mask.cpu().numpy(), base.prob8.cpu().numpy(), 20, 20)
    assert np.array_equal(pred.mask.cpu().numpy(), want_mask) and pred.counts.tolist() == want_counts
    assert pred.counts[2] == 0 and int(pred.regions.abstain_contacts.sum().item()) == 0 and pred.cleanup == done


def test_predict_cli_with_regions(whole, tmp_path):
    from PIL import Image

    w = whole
    ck = tmp_path / "checkpoint"
    ck.mkdir()
    torch.save({"net": w["state"]}, ck / "model_epoch1.pth")
    src = tmp_path / "region.png"
    Image.fromarray(w["image"]).save(src)
    common = ["--input", str(src), "--model_dir", str(ck), "--model_arch", "UNet_B", "--selective", "1", "--tile", "160",
              "--halo", "56", "--batch_size", "4", "--cut_off", repr(w["kw"]["cut_off"]), "--s_cut_off",
              repr(w["kw"]["s_cut_off"])]
    out = tmp_path / "out"
    doc = PR.predict_files(PR.parse_arguments(common + [
        "--save_dir", str(out), "--regions", "1", "--min_region", str(w["min_region"]), "--fill_holes",
        str(w["fill_holes"])]))
    pred = PR.predict_image(w["net"], w["image"], batch_size=4, regions=True, min_region=w["min_region"],
                            fill_holes=w["fill_holes"], **w["kw"])
    on_disk = json.load(open(out / "predict.json"))
    assert on_disk == json.loads(json.dumps(doc))
    rec = on_disk["images"][0]
    assert rec["regions"] == len(pred.regions) and rec["largest_region_area"] == int(pred.regions.area.max().item())
    assert rec["cleanup"] == pred.cleanup and rec["cleanup"]["removed_regions"] >= 1 and rec["cleanup"]["filled_holes"] >= 1
    assert rec["counts"] == dict(zip(PR.COUNT_NAMES, pred.counts.tolist()))
    assert np.array_equal(np.array(Image.open(out / "region_mask.png")), pred.mask.cpu().numpy())
    rows = list(csv.reader(open(out / "region_regions.csv")))
    assert rows[0] == list(PR.REGION_COLUMNS) + ["centroid_y", "centroid_x", "mean_prob"]
    want = pred.regions.rows()
    assert len(rows) == 1 + len(want)
    for line, r in zip(rows[1:], want):
        assert [int(v) for v in line[:10]] == [r[c] for c in PR.REGION_COLUMNS]
        assert [float(v) for v in line[10:]] == [r["sum_y"] / r["area"], r["sum_x"] / r["area"], r["prob_sum"] / (255 * r["area"])]
    # without the flags: no new file, no new key, the plain mask
    plain_dir = tmp_path / "plain"
    plain = PR.predict_files(PR.parse_arguments(common + ["--save_dir", str(plain_dir)]))
    assert not (plain_dir / "region_regions.csv").exists()
    assert list(plain["images"][0]) == ["input", "height", "width", "tile", "halo", "grid", "tiles", "counts",
                                        "tumor_fraction_of_selected", "coverage", "unanimous_fraction"]
    assert np.array_equal(np.array(Image.open(plain_dir / "region_mask.png")), w["mask"])
    assert {k: rec[k] for k in ("height", "width", "grid", "tiles")} == {k: plain["images"][0][k] for k in
                                                                          ("height", "width", "grid", "tiles")}
