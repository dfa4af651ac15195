"""The tissue mask of whole-image prediction on the GPU: the three kernels against numpy
(tests/_tissue_ref.py), bit for bit; `predict_image(..., tissue=True)` on the fixed half-glass image against the
run without it, on the kept and on the skipped pixels; test-time augmentation against tests/_tta_ref.py's
reduction of tissue-skipping plain predictions; region clean-up; and the predict CLI's files."""
import json

import numpy as np
import pytest
import torch

import selectivenet_for_semantic_segmentation_binary_amd as S
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR
from tests import _predict_ref as R
from tests import _tissue_ref as T
from tests import _tta_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
SIZES = [(1, 9), (37, 53)]


def dev(a):
    return torch.tensor(np.array(a, order="C"), device=DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def padded(view):
    """The whole plane behind tissue_plane's [H,W] view: rows of W rounded up to 4 bytes."""
    H, W = view.shape
    pitch = -(-W // 4) * 4
    assert view.stride() == (pitch, 1)
    return torch.as_strided(view, (H, pitch), (pitch, 1))


def pitched(a, pitch):
    """A [H,W] view with rows of `pitch` bytes, the rest of each row filled with 255 (never to be counted)."""
    H, W = a.shape
    base = torch.full((H, pitch), 255, dtype=torch.uint8, device=DEV)
    base[:, :W] = dev(a)
    return base[:, :W]


# ----------------------------------------------------------------------------- tissue_plane
def edge_image(H, W, bright, spread, seed):
    """RGB whose minimum lands on bright - 1, bright, bright + 1 and whose max - min on spread, spread + 1 (and on
    0 and anything), in every combination that fits into a byte."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lo = np.clip(np.where(rng.random((H, W)) < 0.7, bright + rng.integers(-1, 2, (H, W)), rng.integers(0, 256, (H, W))), 0, 255)
    d = np.where(rng.random((H, W)) < 0.7, spread + rng.integers(-1, 2, (H, W)), rng.integers(0, 256, (H, W)))
    d = np.where(rng.random((H, W)) < 0.1, 0, d)
    hi = np.clip(lo + np.clip(d, 0, 255), 0, 255)
    mid = rng.integers(lo, hi + 1)
    px = np.stack([lo, mid, hi], axis=2)
    return np.ascontiguousarray(rng.permuted(px, axis=2).astype(np.uint8))  # min and max in any channel


@pytest.mark.parametrize("bright,spread", [(237, 11), (0, 0), (0, 255), (255, 0), (255, 255), (128, 30)])
@pytest.mark.parametrize("H,W", SIZES)
def test_tissue_plane_equals_numpy(H, W, bright, spread):
    image = edge_image(H, W, bright, spread, seed=H * 1000 + bright + spread)
    want = T.plane_of(image, bright, spread)
    px = image.astype(np.int64)
    lo, d = px.min(axis=2), px.max(axis=2) - px.min(axis=2)
    if (H, W) == (37, 53):  # the edges are met, on either side
        for v in {max(bright - 1, 0), bright, min(bright + 1, 255)}:
            assert (lo == v).any(), v
        low = max(bright - 1, 0)  # the smallest minimum drawn on purpose: what fits into a byte above it
        assert (d == spread).any() or low + spread > 255
        assert (d == spread + 1).any() or low + spread + 1 > 255
        assert bright == 0 and spread == 255 or (want == 0).any() and (want == 255).any()
    got = PR.tissue_plane(dev(image), bright, spread)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W)
    assert np.array_equal(got.cpu().numpy(), want)
    whole = padded(got).cpu().numpy()
    assert whole.shape[1] % 4 == 0 and whole.shape[1] > W and not whole[:, W:].any()  # the padding bytes are 0


def test_tissue_plane_without_padding_and_defaults():
    image = edge_image(5, 8, PR.TISSUE_BRIGHT, PR.TISSUE_SPREAD, seed=8)  # pitch == W: every group is a 12-B load
    got = PR.tissue_plane(dev(image))
    assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), T.plane_of(image))
    assert S.tissue_plane is PR.tissue_plane


# ----------------------------------------------------------------------------- tile_tissue_counts
def sparse_plane(H, W, seed, k=7):
    rng = np.random.Generator(np.random.PCG64(seed))
    plane = np.zeros((H, W), np.uint8)
    plane.reshape(-1)[rng.choice(H * W, min(k, H * W // 3), replace=False)] = 255
    plane[0, 0] = 255  # a corner is reflected in both directions
    return plane


def window_cases():
    far = np.array([(-8, -8), (0, 0), (-40, 60), (-100, -131), (13, 21)], np.int32)  # several folds either way
    yield 1, 9, 24, far
    for tile in (24, 40):
        origins = R.grid_of(37, 53, tile, 8)[2].astype(np.int32)
        yield 37, 53, tile, np.concatenate([origins, far])


@pytest.mark.parametrize("H,W,tile,origins", list(window_cases()), ids=lambda v: str(v) if np.isscalar(v) else "origins")
def test_tile_tissue_counts_equal_numpy(H, W, tile, origins):
    plane = sparse_plane(H, W, seed=H + W + tile)
    full = np.full((H, W), 255, np.uint8)
    seen = set()
    for flip in range(4):
        want = T.window_counts(plane, origins, tile, tile, flip)
        got = PR.tile_tissue_counts(dev(plane), dev(origins), tile, tile, flip)  # rows of W bytes: no alignment
        assert got.dtype == torch.int32 and got.cpu().numpy().tolist() == want.tolist(), flip
        got = PR.tile_tissue_counts(pitched(plane, 64), dev(origins), tile, tile, flip)  # a view with padded rows
        assert got.cpu().numpy().tolist() == want.tolist(), flip
        seen.add(tuple(want.tolist()))
        got = PR.tile_tissue_counts(pitched(full, 56), dev(origins), tile, tile, flip)
        assert (got.cpu().numpy() == tile * tile).all(), flip
    assert len(seen) == (4 if H > 1 else 2)  # the flips differ
    # reflected copies show: some window counts more than its part inside the image holds
    framed = np.pad(plane, 256)
    inside = [np.count_nonzero(framed[y0 + 256:y0 + 256 + tile, x0 + 256:x0 + 256 + tile]) for y0, x0 in origins]
    assert (T.window_counts(plane, origins, tile, tile) > np.array(inside)).any()
    # a rectangular window, into a slice of a larger buffer
    buf = torch.full((len(origins) + 2,), -7, dtype=torch.int32, device=DEV)
    PR.tile_tissue_counts(dev(plane), dev(origins), 8, tile, 3, out=buf[1:-1])
    assert buf.cpu().numpy().tolist() == [-7] + T.window_counts(plane, origins, 8, tile, 3).tolist() + [-7]
    # tissue_plane's own view is taken as it is
    image = np.repeat(np.where(plane[:, :, None] != 0, 90, 250), 3, axis=2).astype(np.uint8)
    got = PR.tile_tissue_counts(PR.tissue_plane(dev(image)), dev(origins), tile, tile, 1)
    assert got.cpu().numpy().tolist() == T.window_counts(plane, origins, tile, tile, 1).tolist()


# ----------------------------------------------------------------------------- tissue_class_counts
def test_tissue_class_counts_equal_numpy():
    H, W = 37, 53
    rng = np.random.Generator(np.random.PCG64(53))
    mask = rng.choice(np.array([0, 127, 255], np.uint8), (H, W), p=[0.5, 0.2, 0.3])
    plane = rng.choice(np.array([0, 255], np.uint8), (H, W))
    want = TR.counts_of(mask[plane != 0])
    assert min(want[:3]) > 100 and want[3] == int((plane != 0).sum()) < H * W
    for m, p in ((dev(mask), dev(plane)), (pitched(mask, 56), pitched(plane, 56)), (pitched(mask, 61), dev(plane))):
        assert PR.tissue_class_counts(m, p).cpu().numpy().tolist() == want
    full = dev(np.full((H, W), 255, np.uint8))
    assert PR.tissue_class_counts(dev(mask), full).cpu().numpy().tolist() == TR.counts_of(mask)
    assert PR.tissue_class_counts(dev(mask), dev(np.zeros((H, W), np.uint8))).cpu().numpy().tolist() == [0, 0, 0, 0]
    acc = torch.tensor([1, 2, 3, 4], dtype=torch.int64, device=DEV)  # added into the caller's words
    PR.tissue_class_counts(dev(mask), dev(plane), acc)
    assert acc.cpu().numpy().tolist() == [a + b for a, b in zip([1, 2, 3, 4], want)]


# ----------------------------------------------------------------------------- whole path
KW = dict(tile=T.TILE, halo=T.HALO, batch_size=4)
NAMES = ("logit", "selection", "mask", "prob8")


def fields(pred, names=NAMES):
    return {k: getattr(pred, k).cpu().numpy() for k in names}


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(
        bits(a) if a.dtype == F32 else a, bits(b) if b.dtype == F32 else b)


@pytest.fixture(scope="module")
def whole():
    """The calibrated network of tests/test_gpu_predict.py, the fixed half-glass image (35 tiles of 160, halo 56),
    its plane by numpy, and the run without the tissue rule (computed once)."""
    state = R.state_dict_of(*R.calibrated_state())
    net = S.UNet_B("RGB", selective=True)
    net.load_state_dict(state)
    net = net.to(DEV).eval()
    image = T.fixed_image()
    return {"state": state, "net": net, "image": image, "plane": T.plane_of(image), "base": PR.predict_image(net, image, **KW)}


def check_against_base(pred, base, cover, shape):
    """On the pixels of kept tiles the run without the rule, bit for bit; on the others the constants."""
    got, ref = fields(pred), fields(base)
    H, W = shape
    assert got["logit"].shape == (H, W) and cover.any() and (~cover).any()
    with np.errstate(invalid="ignore"):
        d = max(float(np.abs(got[k][cover] - ref[k][cover]).max()) for k in ("logit", "selection"))
    print(f"kept pixels against the run without the tissue rule: max |difference| {d}")
    for k in NAMES:
        assert same(got[k][cover], ref[k][cover]), k
    assert (got["logit"][~cover] == -np.inf).all() and (got["selection"][~cover] == np.inf).all()
    assert not got["mask"][~cover].any() and not got["prob8"][~cover].any()
    assert np.isfinite(ref["logit"]).all() and np.isfinite(ref["selection"]).all()
    return got


@pytest.mark.parametrize("min_pixels", [1, 5])
def test_tissue_skips_glass_tiles_and_keeps_the_rest_as_it_was(whole, min_pixels):
    w = whole
    H, W = w["image"].shape[:2]
    kept = T.kept_of(w["image"], 0, min_pixels)
    assert 0 < kept.sum() < kept.size == 35  # the member both keeps and skips
    pred = PR.predict_image(w["net"], w["image"], tissue=True, tissue_min_pixels=min_pixels, **KW)
    assert len(pred.tiles_kept) == 1 and pred.tiles_kept[0].dtype == bool and np.array_equal(pred.tiles_kept[0], kept)
    assert (pred.tiles_forwarded, pred.tiles_total) == (int(kept.sum()), 35)
    got = check_against_base(pred, w["base"], T.core_cover((H, W), kept), (H, W))
    assert pred.counts.tolist() == TR.counts_of(got["mask"]) and int(pred.counts[:3].sum()) == int(pred.counts[3]) == H * W
    plane = pred.tissue.cpu().numpy()
    assert plane.dtype == np.uint8 and np.array_equal(plane, w["plane"])
    assert pred.tissue_counts.dtype == np.int64 and pred.tissue_counts.tolist() == TR.counts_of(got["mask"][plane != 0])
    tc = pred.tissue_counts
    assert min(tc[:3]) > 0 and pred.tumor_fraction_of_tissue == float(tc[1]) / float(tc[0] + tc[1])
    assert pred.tumor_fraction_of_tissue > pred.tumor_fraction  # glass counts as selected background
    assert w["base"].tissue is None and w["base"].tissue_counts is None and w["base"].tiles_kept is None


def test_an_all_tissue_image_is_the_run_without_the_rule(whole):
    w = whole
    crop = np.ascontiguousarray(w["image"][:, :148])
    a = PR.predict_image(w["net"], crop, **KW)
    b = PR.predict_image(w["net"], crop, tissue=True, **KW)
    assert b.tiles_kept[0].all() and b.tiles_forwarded == b.tiles_total == b.plan.n == 20
    fa, fb = fields(a), fields(b)
    for k in NAMES:
        assert same(fa[k], fb[k]), k
    assert a.counts.tolist() == b.counts.tolist() == b.tissue_counts.tolist() and bool(b.tissue.all())


def test_the_default_run_launches_nothing_new(whole):
    """The library calls of a run, by name: without the rule none of the tissue calls; with it, on an all-tissue
    image, the same calls in the same order plus the plane, the window counts and the class counts."""
    from selectivenet_for_semantic_segmentation_binary_amd import _lib as K

    w = whole
    crop = np.ascontiguousarray(w["image"][:, :148])
    names = []

    def hook(name, args, fn):
        names.append(name)
        return fn()

    PR.predict_image(w["net"], crop, **KW)  # whatever the engine prepares on the first forward of a shape is done
    K.set_call_hook(hook)
    try:
        PR.predict_image(w["net"], crop, **KW)
        off = list(names)
        del names[:]
        PR.predict_image(w["net"], crop, tissue=True, **KW)
        on = list(names)
    finally:
        K.set_call_hook(None)
    assert off.count("selunet_tile_gather") == off.count("selunet_tile_stitch") == 5 and not any("tissue" in n for n in off)
    assert [n for n in on if "tissue" not in n] == off
    assert [n for n in on if "tissue" in n] == ["selunet_tissue_plane", "selunet_tile_tissue_counts",
                                                "selunet_tissue_class_counts"]
    assert on.index("selunet_tile_tissue_counts") < on.index("selunet_tile_gather")  # decided before the first forward


def test_an_all_glass_image_runs_no_forward(whole):
    image = T.glass((40, 40, 3), 5)

    class Refusing(torch.nn.Module):  # the network's parameters, but any forward is an error
        selective = True

        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, x):
            raise AssertionError("a forward ran")

    pred = PR.predict_image(Refusing(whole["net"]).eval(), image, tissue=True, **KW)
    assert pred.tiles_forwarded == 0 and pred.tiles_total == 1 and not pred.tiles_kept[0].any()
    assert pred.counts.tolist() == [1600, 0, 0, 1600] and pred.tissue_counts.tolist() == [0, 0, 0, 0]
    assert np.isnan(pred.tumor_fraction_of_tissue) and pred.tumor_fraction == 0.0 and pred.coverage == 1.0
    assert (pred.logit == -np.inf).all() and (pred.selection == np.inf).all()
    assert not pred.mask.any() and not pred.prob8.any() and not pred.tissue.any()
    for tta in ("flips", "d4"):
        pred = PR.predict_image(Refusing(whole["net"]).eval(), image, tissue=True, tta=tta, **KW)
        assert pred.tiles_forwarded == 0 and pred.tiles_total == pred.members and pred.counts.tolist() == [1600, 0, 0, 1600]
        assert (pred.logit == -np.inf).all() and not pred.votes.any() and (pred.sel_votes == pred.members).all()


# ----------------------------------------------------------------------------- test-time augmentation
@pytest.fixture(scope="module")
def ensemble(whole):
    """tests/_tta_ref.py's reduction of eight tissue-skipping plain predictions (batches of 4), computed once. The
    cut-offs are set from that reference as tests/test_gpu_predict_tta.py sets them — sigmoid of the median of
    the finite part of the D4 mean plane, per head — so that all three mask classes occur."""
    w = whole
    kept = []

    def plain(image):
        p = PR.predict_image(w["net"], image, tissue=True, **KW)
        kept.append(p.tiles_kept[0])
        return p.logit.cpu().numpy(), p.selection.cpu().numpy()

    mem = TR.member_planes(plain, w["image"], 8)
    cuts = []
    for i in range(2):
        mean = TR.reduce_members([m[i] for m in mem]).astype(np.float64)
        cuts.append(float(1.0 / (1.0 + np.exp(-np.median(mean[np.isfinite(mean)])))))
    return {"members": mem, "kept": kept, "kw": dict(KW, cut_off=cuts[0], s_cut_off=cuts[1]),
            "t_out": F32(MT.logit_threshold("eval", cuts[0])), "t_sel": F32(MT.logit_threshold("eval", cuts[1]))}


@pytest.mark.parametrize("tta", ["flips", "d4"])
def test_tta_with_tissue_equals_the_reduction_of_tissue_skipping_plain_calls(whole, ensemble, tta):
    w, e = whole, ensemble
    H, W = w["image"].shape[:2]
    members = TR.MEMBERS[tta]
    mem = e["members"][:members]
    outs, sels = [m[0] for m in mem], [m[1] for m in mem]
    ref = {"logit": TR.reduce_members(outs), "selection": TR.reduce_members(sels), "votes": TR.votes_of(outs, e["t_out"]),
           "sel_votes": TR.votes_of(sels, e["t_sel"])}
    ref["mask"] = TR.mask_of(ref["logit"], ref["selection"], e["t_out"], e["t_sel"])
    pred = PR.predict_image(w["net"], w["image"], tta=tta, tissue=True, **e["kw"])
    got = fields(pred, NAMES + ("votes", "sel_votes"))
    assert pred.members == members and got["logit"].shape == (H, W)
    assert not np.isnan(ref["logit"]).any() and not np.isnan(ref["selection"]).any()
    for k in ("logit", "selection", "mask", "votes", "sel_votes"):
        assert same(got[k], ref[k]), k
    assert pred.counts.tolist() == TR.counts_of(ref["mask"]) and int(pred.counts[3]) == H * W
    # every member decides on its own tiling, and both keeps and skips
    assert len(pred.tiles_kept) == members
    covers = []
    for k in range(members):
        kept = T.kept_of(w["image"], k)
        assert 0 < kept.sum() < kept.size and np.array_equal(pred.tiles_kept[k], kept), k
        assert np.array_equal(e["kept"][k], kept), k  # the plain calls of the reference skipped the same tiles
        covers.append(TR.T_inv(k, T.core_cover(TR.T(k, w["plane"]).shape, kept)))
    assert pred.tiles_total == 35 * members and pred.tiles_forwarded == sum(int(k.sum()) for k in pred.tiles_kept)
    # a pixel that any member skipped: mean logit -inf, mean selection +inf, background, no tumor vote of that member
    every = np.all(covers, axis=0)
    assert every.any() and (~every).any()
    assert (got["logit"][~every] == -np.inf).all() and (got["selection"][~every] == np.inf).all()
    assert not got["mask"][~every].any() and not got["prob8"][~every].any() and (got["votes"][~every] < members).all()
    assert np.isfinite(got["logit"][every]).all() and min(pred.counts[:3]) > 0
    # pixels no member skipped: the run without the rule, bit for bit
    base = fields(PR.predict_image(w["net"], w["image"], tta=tta, **e["kw"]), NAMES + ("votes", "sel_votes"))
    for k in base:
        assert same(got[k][every], base[k][every]), k
    plane = pred.tissue.cpu().numpy()
    assert np.array_equal(plane, w["plane"]) and pred.tissue_counts.tolist() == TR.counts_of(got["mask"][plane != 0])


# ----------------------------------------------------------------------------- regions and clean-up
def test_tissue_counts_are_those_of_the_cleaned_mask(whole):
    w = whole
    raw = PR.predict_image(w["net"], w["image"], tissue=True, **KW)
    pred = PR.predict_image(w["net"], w["image"], tissue=True, regions=True, min_region=50, **KW)
    assert pred.regions is not None and pred.cleanup["removed_pixels"] > 0
    mask, plane = pred.mask.cpu().numpy(), pred.tissue.cpu().numpy()
    assert pred.counts.tolist() == TR.counts_of(mask) and np.array_equal(plane, w["plane"])
    assert pred.tissue_counts.tolist() == TR.counts_of(mask[plane != 0])
    assert pred.tissue_counts.tolist() != raw.tissue_counts.tolist() and pred.tissue_counts[3] == raw.tissue_counts[3]
    assert np.array_equal(pred.tiles_kept[0], raw.tiles_kept[0]) and pred.tiles_forwarded == raw.tiles_forwarded


# ----------------------------------------------------------------------------- CLI
def test_predict_cli_with_and_without_tissue(whole, tmp_path):
    from PIL import Image

    w = whole
    ck = tmp_path / "checkpoint"
    ck.mkdir()
    torch.save({"net": w["state"]}, ck / "model_epoch1.pth")
    src = tmp_path / "slide.png"
    Image.fromarray(w["image"]).save(src)
    common = ["--input", str(src), "--model_dir", str(ck), "--model_arch", "UNet_B", "--selective", "1", "--tile", "160",
              "--halo", "56", "--batch_size", "4"]
    doc = PR.predict_files(PR.parse_arguments(common + ["--save_dir", str(tmp_path / "on"), "--tissue", "1",
                                                        "--tissue_min_pixels", "5"]))
    on_disk = json.load(open(tmp_path / "on" / "predict.json"))
    assert on_disk == json.loads(json.dumps(doc))
    assert (on_disk["tissue_bright"], on_disk["tissue_spread"], on_disk["tissue_min_pixels"]) == (237, 11, 5)
    assert list(on_disk)[-1] == "images"
    assert np.array_equal(np.array(Image.open(tmp_path / "on" / "slide_tissue.png")), w["plane"])
    mask = np.array(Image.open(tmp_path / "on" / "slide_mask.png"))
    rec = on_disk["images"][0]
    tc = TR.counts_of(mask[w["plane"] != 0])
    assert rec["tissue_pixels"] == tc[3] == int((w["plane"] != 0).sum()) and rec["tissue_counts"] == dict(zip(PR.COUNT_NAMES, tc))
    assert rec["tumor_fraction_of_tissue"] == tc[1] / (tc[0] + tc[1]) and rec["counts"] == dict(zip(PR.COUNT_NAMES, TR.counts_of(mask)))
    assert (rec["tiles_forwarded"], rec["tiles_total"]) == (25, 35)
    # --tissue 0, and no flag at all: the keys of the document and of the record are what they were
    for name, flags in (("off", ["--tissue", "0"]), ("plain", [])):
        off = PR.predict_files(PR.parse_arguments(common + ["--save_dir", str(tmp_path / name)] + flags))
        assert list(off) == ["checkpoint", "selective", "input_type", "cut_off", "s_cut_off", "single_scale", "tta", "images"]
        assert list(off["images"][0]) == ["input", "height", "width", "tile", "halo", "grid", "tiles", "counts",
                                          "tumor_fraction_of_selected", "coverage", "unanimous_fraction"]
        assert not (tmp_path / name / "slide_tissue.png").exists()
        assert sorted(p.name for p in (tmp_path / name).iterdir()) == ["predict.json", "slide_mask.png", "slide_prob.png",
                                                                       "slide_select.png"]
    assert open(tmp_path / "off" / "predict.json").read().replace(str(tmp_path / "off"), "") == \
        open(tmp_path / "plain" / "predict.json").read().replace(str(tmp_path / "plain"), "")
