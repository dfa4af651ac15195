"""Macenko stain normalisation on the GPU: the four kernels against numpy (tests/_stain_ref.py), bit
for bit, at sizes that meet every path of their pixel walk; images without a stained pixel, with skipped pixels and
with concentrations and indices beyond both clamps; the argument rules; `stain.normalize` against the restated
pipeline; `predict_image(stain=)` against the prediction of the separately normalised image; and the predict CLI."""
import json

import numpy as np
import pytest
import torch

import selectivenet_for_semantic_segmentation_binary_amd as S
import selectivenet_for_semantic_segmentation_binary_amd.layout as L
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR
from selectivenet_for_semantic_segmentation_binary_amd import stain as ST
from tests import _stain_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BQ = R.beta_q_of()
# 1 x 1; 5 x 7: no row is a multiple of 4 pixels and rows start at every byte alignment; 64 x 64: whole groups only;
# 37 x 1031: long ragged rows; 300 x 517: 300 * 130 = 39000 groups of four pixels.
SHAPES = [(1, 1), (5, 7), (64, 64), (37, 1031), (300, 517)]
# The launchers' grids are capped at 2048 workgroups of 256 threads (STAIN_GRID), and
# 39000 groups need 153: read off csrc/stain.hip, no image a test can afford makes a default grid stride twice.
# So 300 x 517 runs a second time under IO_GRID = 16, the option every grid-stride launcher takes its cap from
# (common.h io_grid): 4096 threads walk 39000 groups in 10 passes, the last one ragged (39000 = 9 * 4096 + 2136).
CAPPED = (300, 517, 16)


def dev(a):
    return torch.tensor(np.array(a, order="C"), device=DEV)


@pytest.fixture(scope="module")
def tables():
    return {"od": dev(R.OD_Q), "exp": dev(R.EXP_Q), "dirs": dev(R.DIRS)}


@pytest.fixture(scope="module")
def seed0():
    """The 96 x 128 synthetic image of seed 0 and its restated pipeline: the B, P_q and T_q every shape is run with."""
    image = R.synthetic_he(96, 128, seed=0)
    out, fit = R.normalize_int(image)
    assert fit["applied"]
    return {"image": image, "out": out, "fit": fit}


def words(n):
    return torch.zeros(n, dtype=torch.int64, device=DEV)  # uint64 bits


def host(t):
    return t.cpu().numpy().view(np.uint64)


def i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data


def run_moments(t, img, beta_q=BQ, acc=None):
    acc = words(10) if acc is None else acc
    K.call("selunet_stain_moments", K.ptr(img), img.shape[0], img.shape[1], K.ptr(t["od"]), beta_q, K.ptr(acc), K.stream_ptr())
    return acc


def run_angle(t, img, B, beta_q=BQ, acc=None):
    acc = words(R.K + 1) if acc is None else acc
    keep, p = i32(B)
    K.call("selunet_stain_angle_hist", K.ptr(img), img.shape[0], img.shape[1], K.ptr(t["od"]), beta_q, p, K.ptr(t["dirs"]),
           K.ptr(acc), K.stream_ptr())
    return acc


def run_conc(t, img, P_q, beta_q=BQ, acc=None):
    acc = words(2 * R.CB) if acc is None else acc
    keep, p = i32(P_q)
    K.call("selunet_stain_conc_hist", K.ptr(img), img.shape[0], img.shape[1], K.ptr(t["od"]), beta_q, p, K.ptr(acc),
           K.stream_ptr())
    return acc


def run_apply(t, img, T_q, exp=None, out=None):
    exp = t["exp"] if exp is None else exp
    out = torch.full_like(img, 7) if out is None else out
    keep, p = i32(T_q)
    K.call("selunet_stain_apply", K.ptr(img), img.shape[0], img.shape[1], K.ptr(t["od"]), p, K.ptr(exp), exp.numel(), K.ptr(out),
           K.stream_ptr())
    return out


# ----------------------------------------------------------------------------- the four kernels
_REF = {}


def reference(seed0, H, W):
    """The four passes by numpy on the H x W synthetic image, computed once per shape."""
    if (H, W) not in _REF:
        image = R.synthetic_he(H, W, seed=H + W)
        if (H, W) == (1, 1):
            image[0, 0] = (120, 40, 130)  # the one pixel is stained
        f = seed0["fit"]
        _REF[H, W] = {"image": image, "moments": R.moments(image, BQ),
                      "angle": R.angle_hist(image, BQ, f["B"], check_monotone=H * W < 50000),
                      "conc": R.conc_hist(image, BQ, f["P_q"]), "apply": R.apply_int(image, f["T_q"])}
    return _REF[H, W]


def check_kernels(tables, seed0, H, W):
    ref, f = reference(seed0, H, W), seed0["fit"]
    img = dev(ref["image"])
    assert int(ref["moments"][0]) >= 1
    assert host(run_moments(tables, img)).tolist() == ref["moments"].tolist()
    got = host(run_angle(tables, img, f["B"]))
    assert got.tolist() == ref["angle"].tolist() and int(got.sum()) == int(ref["moments"][0])
    got = host(run_conc(tables, img, f["P_q"])).reshape(2, R.CB)
    assert np.array_equal(got, ref["conc"]) and got.sum(axis=1).tolist() == [int(ref["moments"][0])] * 2
    assert np.array_equal(run_apply(tables, img, f["T_q"]).cpu().numpy(), ref["apply"])


@pytest.mark.parametrize("H,W", SHAPES)
def test_kernels_equal_numpy(tables, seed0, H, W):
    check_kernels(tables, seed0, H, W)


def test_kernels_equal_numpy_where_the_loops_iterate(tables, seed0):
    H, W, grid = CAPPED
    assert H * -(-W // 4) > 9 * grid * 256 and H * -(-W // 4) % (grid * 256) != 0  # ten passes, the last ragged
    prev = K.set_option("IO_GRID", grid)
    try:
        check_kernels(tables, seed0, H, W)
    finally:
        K.set_option("IO_GRID", prev)


def test_the_statistics_calls_add_into_their_words(tables, seed0):
    a, b = seed0["image"], R.synthetic_he(40, 52, seed=9)
    f = seed0["fit"]
    acc = run_moments(tables, dev(b), acc=run_moments(tables, dev(a)))
    assert host(acc).tolist() == (R.moments(a, BQ) + R.moments(b, BQ)).tolist()
    acc = run_angle(tables, dev(b), f["B"], acc=run_angle(tables, dev(a), f["B"]))
    assert host(acc).tolist() == (R.angle_hist(a, BQ, f["B"]) + R.angle_hist(b, BQ, f["B"])).tolist()
    acc = run_conc(tables, dev(b), f["P_q"], acc=run_conc(tables, dev(a), f["P_q"]))
    assert host(acc).tolist() == (R.conc_hist(a, BQ, f["P_q"]) + R.conc_hist(b, BQ, f["P_q"])).reshape(-1).tolist()


def test_an_image_without_a_stained_pixel(tables, seed0):
    image = np.full((9, 13, 3), 255, np.uint8)
    image[2, 3] = (255, 10, 10)  # one channel at no density: not stained
    f = seed0["fit"]
    assert not host(run_moments(tables, dev(image))).any()
    assert not host(run_angle(tables, dev(image), f["B"])).any()
    assert not host(run_conc(tables, dev(image), f["P_q"])).any()
    assert np.array_equal(run_apply(tables, dev(image), f["T_q"]).cpu().numpy(), R.apply_int(image, f["T_q"]))
    out, info = ST.normalize(dev(image))
    assert info["applied"] is False and "0 stained" in info["reason"] and np.array_equal(out.cpu().numpy(), image)


def skipped_image():
    """40 x 52, red-dominated: the density of R runs over (1, 3) and that of B against it, so the first
    eigenvector has a negative B component; five pixels of pure blue, densities (0.2, 0.2, 5.5), project onto it
    with x <= 0."""
    rng = np.random.Generator(np.random.PCG64(5))
    t = rng.random((40, 52))
    od = np.stack([1.0 + 2.0 * t, 0.5 + 0.2 * rng.random((40, 52)), 1.5 - 1.0 * t], axis=2)
    od[3, 4:9] = (0.2, 0.2, 5.5)
    return np.clip(np.rint(255.0 * np.exp(-od)), 0, 255).astype(np.uint8)


def test_pixels_with_x_not_positive_are_skipped(tables):
    image = skipped_image()
    assert (R.OD_Q[image[3, 4]] >= BQ).all()  # the blue pixels are stained
    ref = R.fit_int([image])
    assert ref["skipped"] == 5 and ref["B"][0][2] < 0
    got = host(run_angle(tables, dev(image), ref["B"]))
    assert got.tolist() == [int(v) for v in ref["angle_hist"]] and int(got[R.K]) == 5
    fit = ST.fit(dev(image))
    assert fit.skipped == 5 and fit.n_stained == ref["n_stained"]
    assert np.array_equal(fit.HE, ref["HE"]) and np.array_equal(fit.maxC, ref["maxC"])


def test_both_clamps_of_the_concentration_histogram(tables, seed0):
    image = seed0["image"]
    P_q = np.rint(4096.0 * np.array([[3.0, 0.0, 0.0], [-1.0, 0.0, 1.0]])).astype(np.int32)
    raw = R.stained_od(image, BQ) @ P_q.astype(np.int64).T >> 17
    assert (raw[:, 0] >= R.CB).any() and (raw[:, 1] < 0).any()  # above 8 and below 0
    ref = R.conc_hist(image, BQ, P_q)
    assert ref[0, R.CB - 1] > 0 and ref[1, 0] > 0
    assert np.array_equal(host(run_conc(tables, dev(image), P_q)).reshape(2, R.CB), ref)


def test_apply_clamps_its_index_at_both_ends(tables, seed0):
    image = seed0["image"]
    T_q = np.rint(16384.0 * np.array([[-2.0, 0.0, 0.0], [0.0, 3.0, 0.0], [1.0, 1.0, 1.0]])).astype(np.int32)
    idx = (R.od_of(image) @ T_q.astype(np.int64).T + (1 << 15)) >> 16
    assert (idx < 0).any() and (idx >= len(R.EXP_Q)).any()
    assert np.array_equal(run_apply(tables, dev(image), T_q).cpu().numpy(), R.apply_int(image, T_q))
    short = R.EXP_Q[:100]  # a shorter table: the clamp is the call's n_exp
    assert np.array_equal(run_apply(tables, dev(image), seed0["fit"]["T_q"], exp=dev(short)).cpu().numpy(),
                          R.apply_int(image, seed0["fit"]["T_q"], short))
    odd = dev(np.concatenate([R.EXP_Q[:1], R.EXP_Q]))[1:]  # a table at an odd address is staged byte by byte
    assert odd.data_ptr() % 4 == 1
    assert np.array_equal(run_apply(tables, dev(image), T_q, exp=odd).cpu().numpy(), R.apply_int(image, T_q))
    assert np.array_equal(ST.apply(dev(image), np.eye(3)).cpu().numpy(), np.maximum(image, 1))  # the identity


def test_argument_checks_answer_with_a_message(tables, seed0):
    img, f = dev(seed0["image"]), seed0["fit"]
    H, W = img.shape[:2]
    out = torch.empty_like(img)
    od, ex = K.ptr(tables["od"]), K.ptr(tables["exp"])
    _, T = i32(f["T_q"])
    big, T_big = i32(np.where(np.eye(3) > 0, 1 << 20, 0))
    s = K.stream_ptr()
    for args, word in (((None, H, W, od, T, ex, len(R.EXP_Q), K.ptr(out), s), "null"),
                       ((K.ptr(img), 0, W, od, T, ex, len(R.EXP_Q), K.ptr(out), s), "height and width"),
                       ((K.ptr(img), H, W, od, T_big, ex, len(R.EXP_Q), K.ptr(out), s), "2\\^20"),
                       ((K.ptr(img), H, W, od, T, ex, len(R.EXP_Q), K.ptr(img), s), "alias")):
        with pytest.raises(K.SelunetError, match=word):
            K.call("selunet_stain_apply", *args)
    acc = words(2 * R.CB)
    keep_p, P_q = i32(f["P_q"])
    keep_b, B = i32(f["B"])
    with pytest.raises(K.SelunetError, match="null"):
        K.call("selunet_stain_moments", None, H, W, od, BQ, K.ptr(acc), s)
    with pytest.raises(K.SelunetError, match="height and width"):
        K.call("selunet_stain_conc_hist", K.ptr(img), 0, W, od, BQ, P_q, K.ptr(acc), s)
    with pytest.raises(K.SelunetError, match="null"):
        K.call("selunet_stain_angle_hist", K.ptr(img), H, W, od, BQ, B, None, K.ptr(acc), s)
    torch.cuda.synchronize()
    assert not host(acc).any()  # nothing was launched


# ----------------------------------------------------------------------------- stain.py on the device
def test_normalize_equals_the_restated_pipeline(seed0):
    image, f = seed0["image"], seed0["fit"]
    out, info = ST.normalize(dev(image))
    assert torch.is_tensor(out) and out.device.type == "cuda" and np.array_equal(out.cpu().numpy(), seed0["out"])
    assert info["applied"] is True and info["HE"] == f["HE"].tolist() and info["maxC"] == f["maxC"].tolist()
    assert (info["n_stained"], info["skipped"]) == (f["n_stained"], f["skipped"]) and info["T"] == f["T"].tolist()
    out_np, info_np = ST.normalize(image)  # a numpy image comes back as one
    assert isinstance(out_np, np.ndarray) and np.array_equal(out_np, seed0["out"]) and info_np == info
    again = ST.fit(out)
    deg = [R.angle_deg(again.HE[:, s], R.TARGET_HE[:, s]) for s in range(2)]
    print(f"re-fitted vectors of the normalised image against the target's: {deg[0]:.3f} deg, {deg[1]:.3f} deg")
    assert max(deg) <= R.REFIT_DEG
    # fit_many on the device: the words of two images in one set
    other = R.synthetic_he(64, 128, seed=7, he=([0.55, 0.76, 0.35], [0.10, 0.95, 0.29]))
    many, ref = ST.fit_many([image, dev(other)]), R.fit_int([image, other])
    assert np.array_equal(many.HE, ref["HE"]) and np.array_equal(many.maxC, ref["maxC"]) and many.n_stained == ref["n_stained"]
    assert S.stain is ST and S.StainFit is ST.StainFit and S.MACENKO_TARGET is ST.MACENKO_TARGET


# ----------------------------------------------------------------------------- predict_image
KW = dict(tile=64, halo=8, allow_small_halo=True, batch_size=3)  # the smallest halo of tests/test_gpu_predict.py
NAMES = ("logit", "selection", "mask", "prob8")


def same(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    view = (lambda v: np.ascontiguousarray(v).view(np.uint32)) if a.dtype == np.float32 else (lambda v: v)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(view(a), view(b))


@pytest.fixture(scope="module")
def whole():
    """A seeded selective UNet_B and a 96 x 80 synthetic image whose lower right block is glass: 2 x 2 tiles of 64
    with halo 8, the last one's whole window glass."""
    p = L.seeded_params(0, "RGB", True)
    net = S.UNet_B("RGB", selective=True)
    with torch.no_grad():
        for k, t in net.named_parameters():
            t.copy_(torch.tensor(p[k]))
    net = net.to(DEV).eval()
    image = R.synthetic_he(96, 80, seed=11, glass=0.0, shape=(8.0, 8.0), scale=(0.1, 0.06))  # 4421 stained pixels
    image[40:, 24:] = 255  # 56 x 56: the window of the last tile of every flip and transpose of the image
    return {"net": net, "image": image, "target": ST.MACENKO_TARGET}


@pytest.mark.parametrize("tta", ["none", "d4"])
def test_predict_with_stain_is_the_prediction_of_the_normalised_image(whole, tta):
    w = whole
    normalised, info = ST.normalize(w["image"], w["target"])
    assert info["applied"] and not np.array_equal(normalised, w["image"])
    assert np.array_equal(normalised, R.normalize_int(w["image"])[0])
    got = PR.predict_image(w["net"], w["image"], stain=w["target"], tta=tta, **KW)
    ref = PR.predict_image(w["net"], normalised, tta=tta, **KW)
    for k in NAMES + (("votes", "sel_votes") if tta != "none" else ()):
        assert same(getattr(got, k), getattr(ref, k)), k
    assert got.counts.tolist() == ref.counts.tolist() and got.plan.n == 4
    assert got.stain == info and np.array_equal(got.stain_image.cpu().numpy(), normalised)
    assert ref.stain is None and ref.stain_image is None
    # with the tissue rule: the plane and the forwarded tiles are those of the image as it came
    got = PR.predict_image(w["net"], w["image"], stain=w["target"], tissue=True, tta=tta, **KW)
    raw = PR.predict_image(w["net"], w["image"], tissue=True, tta=tta, **KW)
    sep = PR.predict_image(w["net"], normalised, tissue=True, tta=tta, **KW)
    assert same(got.tissue, raw.tissue) and len(got.tiles_kept) == len(raw.tiles_kept) == got.members
    assert all(np.array_equal(a, b) for a, b in zip(got.tiles_kept, raw.tiles_kept))
    assert got.tiles_forwarded == raw.tiles_forwarded == 3 * got.members and got.tiles_total == 4 * got.members
    if all(np.array_equal(a, b) for a, b in zip(sep.tiles_kept, raw.tiles_kept)):  # the same tiles: the same planes
        for k in NAMES:
            assert same(getattr(got, k), getattr(sep, k)), k
    assert np.array_equal(got.stain_image.cpu().numpy(), normalised)


def test_predict_without_stain_is_what_it_was(whole):
    w = whole
    a = PR.predict_image(w["net"], w["image"], **KW)
    b = PR.predict_image(w["net"], w["image"], stain=None, **KW)
    for k in NAMES:
        assert same(getattr(a, k), getattr(b, k)), k
    assert a.counts.tolist() == b.counts.tolist() and b.stain is None and b.stain_image is None
    names = []

    def hook(name, args, fn):
        names.append(name)
        return fn()

    K.set_call_hook(hook)
    try:
        PR.predict_image(w["net"], w["image"], stain=None, **KW)
        off = list(names)
        del names[:]
        PR.predict_image(w["net"], w["image"], stain=w["target"], **KW)
    finally:
        K.set_call_hook(None)
    assert not any("stain" in n for n in off)
    assert [n for n in names if "stain" in n] == ["selunet_stain_moments", "selunet_stain_angle_hist",
                                                  "selunet_stain_conc_hist", "selunet_stain_apply"]
    assert [n for n in names if "stain" not in n] == off and names.index("selunet_stain_apply") < names.index("selunet_tile_gather")


def test_an_image_that_cannot_be_fitted_is_predicted_as_it_is(whole):
    w = whole
    image = np.ascontiguousarray(w["image"][:64, :64])
    image[8:, :] = 255  # 512 pixels of tissue: fewer stained ones than min_stained
    a = PR.predict_image(w["net"], image, stain=w["target"], **KW)
    b = PR.predict_image(w["net"], image, **KW)
    assert a.stain["applied"] is False and "stained" in a.stain["reason"]
    assert np.array_equal(a.stain_image.cpu().numpy(), image)
    for k in NAMES:
        assert same(getattr(a, k), getattr(b, k)), k


# ----------------------------------------------------------------------------- CLI
def test_predict_cli_writes_the_normalised_image_and_the_fit(whole, tmp_path):
    from PIL import Image

    w = whole
    ck = tmp_path / "checkpoint"
    ck.mkdir()
    torch.save({"net": w["net"].state_dict()}, ck / "model_epoch1.pth")
    src = tmp_path / "slide.png"
    Image.fromarray(w["image"]).save(src)
    target = ST.StainFit(R.TARGET_HE, [1.5, 0.9], 123, 4)
    (tmp_path / "target.json").write_text(json.dumps(target.to_json()))
    common = ["--input", str(src), "--model_dir", str(ck), "--model_arch", "UNet_B", "--selective", "1", "--tile", "160",
              "--halo", "56", "--batch_size", "4"]
    doc = PR.predict_files(PR.parse_arguments(common + ["--save_dir", str(tmp_path / "on"), "--stain_norm", "macenko",
                                                        "--stain_target", str(tmp_path / "target.json")]))
    on_disk = json.load(open(tmp_path / "on" / "predict.json"))
    assert on_disk == json.loads(json.dumps(doc)) and list(on_disk)[-1] == "images"
    assert (on_disk["stain_norm"], on_disk["stain_target"], on_disk["stain_beta"]) == ("macenko", target.to_json(), 0.15)
    want, f = R.normalize_int(w["image"], R.TARGET_HE, np.array([1.5, 0.9]))
    assert np.array_equal(np.array(Image.open(tmp_path / "on" / "slide_stain.png")), want)
    rec = on_disk["images"][0]["stain"]
    assert list(rec) == ["applied", "reason", "HE", "maxC", "n_stained", "skipped", "T"]
    assert rec["applied"] is True and rec["reason"] is None and rec["HE"] == f["HE"].tolist() and rec["T"] == f["T"].tolist()
    assert (rec["maxC"], rec["n_stained"], rec["skipped"]) == (f["maxC"].tolist(), f["n_stained"], f["skipped"])
    # the default target, and no flag at all: a plain run's files are what they were
    doc = PR.predict_files(PR.parse_arguments(common + ["--save_dir", str(tmp_path / "default"), "--stain_norm", "macenko"]))
    assert doc["stain_target"] == ST.MACENKO_TARGET.to_json()
    assert np.array_equal(np.array(Image.open(tmp_path / "default" / "slide_stain.png")), R.normalize_int(w["image"])[0])
    off = PR.predict_files(PR.parse_arguments(common + ["--save_dir", str(tmp_path / "off")]))
    assert list(off) == ["checkpoint", "selective", "input_type", "cut_off", "s_cut_off", "single_scale", "tta", "images"]
    assert "stain" not in off["images"][0]
    assert sorted(p.name for p in (tmp_path / "off").iterdir()) == ["predict.json", "slide_mask.png", "slide_prob.png",
                                                                    "slide_select.png"]
    # the stain CLI makes a target from images
    assert ST.main(["fit", "--input", str(src), "--out", str(tmp_path / "fit.json")]) == 0
    made, ref = ST.load_target(tmp_path / "fit.json"), R.fit_int([w["image"]])
    assert np.array_equal(made.HE, ref["HE"]) and np.array_equal(made.maxC, ref["maxC"]) and made.n_stained == ref["n_stained"]
