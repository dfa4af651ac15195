"""Macenko stain normalisation without a GPU: the tables, the integer pipeline of
tests/_stain_ref.py against a float64 textbook Macenko on synthetic H&E images, stain.py's host steps driven
through the numpy passes (`kernels=`), the fallbacks, the JSON form, the CLI flags and the refusals of the four
entry points (host-side, before any launch)."""
import ctypes
import json
import os

import numpy as np
import pytest

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import build as B
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR
from selectivenet_for_semantic_segmentation_binary_amd import stain as ST
from tests import _stain_ref as R

SEEDS = (0, 1, 2)
REF = R.Kernels()


@pytest.fixture(scope="module")
def images():
    return {s: R.synthetic_he(96, 128, seed=s) for s in SEEDS}


@pytest.fixture(scope="module")
def fits(images):
    """Per seed the integer fit, the float fit and both whole pipelines, computed once."""
    out = {}
    for s, im in images.items():
        norm_i, fi = R.normalize_int(im)
        norm_f, ff = R.normalize_float(im)
        out[s] = {"int": fi, "float": ff, "norm_int": norm_i, "norm_float": norm_f}
    return out


# ----------------------------------------------------------------------------- tables
def test_tables():
    od, ex, dirs = ST.od_table(), ST.exp_table(), ST.dir_table()
    assert od.dtype == np.int32 and od.shape == (256,) and od[255] == 0 and od[0] == od[1] == od.max() == 22697
    assert (np.diff(od) <= 0).all()
    assert ex.dtype == np.uint8 and len(ex) == 5676 and ex[0] == 255 and ex[-1] == 1 and (np.diff(ex.astype(int)) <= 0).all()
    assert dirs.dtype == np.int32 and dirs.shape == (1023, 2) and dirs[511].tolist() == [16384, 0]
    assert len(ex) <= K.STAIN_EXP_MAX and (ST.K_BINS, ST.C_BINS) == (K.STAIN_ANGLE_BINS, K.STAIN_CONC_BINS) == (R.K, R.CB)
    for a, b in ((od, R.OD_Q), (ex, R.EXP_Q), (dirs, R.DIRS)):  # numpy's and math's log, exp, cos and sin agree
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert ST.beta_q_of(0.15) == R.beta_q_of(0.15) == 614
    lines = dict(l.split()[1:3] for l in open(os.path.join(os.path.dirname(B.HEADER), "selunet.h"))
                 if l.startswith("#define SELUNET_STAIN_"))
    assert {k: int(v) for k, v in lines.items()} == {"SELUNET_STAIN_ANGLE_BINS": 1024, "SELUNET_STAIN_CONC_BINS": 1024,
                                                     "SELUNET_STAIN_EXP_MAX": 8192}


def test_the_identity_transform_is_exact():
    v = np.arange(256, dtype=np.uint8)
    ramp = np.stack([v, v[::-1], np.roll(v, 77)], axis=1).reshape(4, 64, 3)
    T_q = ST.transform_q(np.eye(3))
    assert T_q.tolist() == (16384 * np.eye(3, dtype=int)).tolist()
    for out in (R.apply_int(ramp, T_q), ST.apply(ramp, np.eye(3), kernels=REF)):
        assert out.dtype == np.uint8 and np.array_equal(out, np.maximum(ramp, 1))  # every v >= 1 to itself, 0 to 1


# ----------------------------------------------------------------------------- against the float64 Macenko
@pytest.mark.parametrize("seed", SEEDS)
def test_integer_fit_is_within_one_bin_of_the_float_fit(images, fits, seed):
    fi, ff = fits[seed]["int"], fits[seed]["float"]
    assert fi["applied"] and fi["n_stained"] == ff["n_stained"] > R.MIN_STAINED and fi["skipped"] == 0
    bin_deg = 180.0 / R.K
    for s in range(2):
        d = R.angle_deg(fi["HE"][:, s], ff["HE"][:, s])
        print(f"seed {seed} stain {s}: integer against float vector {d:.4f} deg (one angular bin {bin_deg:.4f})")
        assert d <= bin_deg
    # a concentration bin, plus what the float fit's own maxC moves when its two angles move by one angular bin
    step = np.pi / R.K
    moved = max(float(np.abs(R.fit_float(images[seed], shift=(a, b))["maxC"] - ff["maxC"]).max())
                for a in (-step, step) for b in (-step, step))
    err = float(np.abs(fi["maxC"] - ff["maxC"]).max())
    print(f"seed {seed}: |maxC int - float| {err:.5f}, bound 1/128 + {moved:.5f}")
    assert err <= 1.0 / 128.0 + moved


@pytest.mark.parametrize("seed", SEEDS)
def test_integer_apply_is_within_one_level_of_the_float_apply(images, fits, seed):
    """The same T on both sides. The index into exp_q is off by at most half a Q10 step from rounding, 0.0005, and
    by the roundings of od_q (2^-13 each) and T_q (2^-15 each) through |T| <= 1 and od <= 5.55, another 0.0009: under
    0.4 of a level at 255 exp(-o) <= 255. exp_q rounds by half a level more, and so does the float side: the two
    bytes differ by less than 2, so by at most 1."""
    T = fits[seed]["int"]["T"]
    assert np.abs(T).max() <= 1.0
    a = fits[seed]["norm_int"].astype(int)
    b = R.apply_float(images[seed], T).astype(int)
    print(f"seed {seed}: integer against float apply with one T: max |difference| {np.abs(a - b).max()} levels")
    assert np.abs(a - b).max() <= 1


def test_whole_integer_pipeline_against_the_whole_float_pipeline(fits):
    """Fit and apply on either side. Measured on seeds 0, 1, 2: 1, 1 and 1 level; asserted: the worst
    of them plus 1."""
    worst = []
    for seed in SEEDS:
        worst.append(int(np.abs(fits[seed]["norm_int"].astype(int) - fits[seed]["norm_float"].astype(int)).max()))
    print(f"integer against float pipeline, seeds {SEEDS}: max |difference| {worst} levels")
    assert max(worst) <= 1 + 1


def test_normalised_image_has_the_targets_stains(fits):
    """Re-fitting the normalised image gives the target's vectors. Measured on seeds 0, 1, 2: hematoxylin 0.012,
    0.018 and 0.011 deg, eosin 1.238, 0.891 and 1.044 deg; asserted: the worst plus 0.5 deg."""
    for seed in SEEDS:
        again = R.fit_int([fits[seed]["norm_int"]])
        deg = [R.angle_deg(again["HE"][:, s], R.TARGET_HE[:, s]) for s in range(2)]
        print(f"seed {seed}: re-fitted vectors against the target's: {deg[0]:.3f} deg, {deg[1]:.3f} deg; maxC {again['maxC']}")
        assert max(deg) <= R.REFIT_DEG
        assert np.abs(again["maxC"] / R.TARGET_MAXC - 1).max() < 0.1


# ----------------------------------------------------------------------------- stain.py's host steps
@pytest.mark.parametrize("seed", SEEDS)
def test_stain_module_over_the_numpy_passes_equals_the_restated_pipeline(images, fits, seed):
    fi = fits[seed]["int"]
    got = ST.fit(images[seed], kernels=REF)
    assert np.array_equal(got.HE, fi["HE"]) and np.array_equal(got.maxC, fi["maxC"])
    assert (got.n_stained, got.skipped) == (fi["n_stained"], fi["skipped"])
    mom = fi["moments"]
    assert np.array_equal(ST.basis_q(*ST.basis_of(mom)), fi["B"]) and np.array_equal(ST.pinv_q(got.HE)[1], fi["P_q"])
    target = ST.MACENKO_TARGET
    assert np.array_equal(target.HE, R.TARGET_HE) and np.array_equal(target.maxC, R.TARGET_MAXC)
    T = ST.transform(got, target)
    assert np.array_equal(T, fi["T"]) and np.array_equal(ST.transform_q(T), fi["T_q"])
    out, info = ST.normalize(images[seed], kernels=REF)
    assert isinstance(out, np.ndarray) and np.array_equal(out, fits[seed]["norm_int"]) and out is not images[seed]
    assert info["applied"] is True and info["reason"] is None and info["T"] == T.tolist()
    assert (info["HE"], info["maxC"], info["n_stained"], info["skipped"]) == (got.HE.tolist(), got.maxC.tolist(),
                                                                             got.n_stained, got.skipped)
    assert json.loads(json.dumps(info)) == info
    assert np.array_equal(ST.apply(images[seed], T, kernels=REF), out)
    # hematoxylin first: the larger R component
    assert got.HE[0, 0] > got.HE[0, 1] and np.allclose(np.linalg.norm(got.HE, axis=0), 1.0)


def test_percentile_bin():
    hist = np.zeros(1024, np.uint64)
    hist[[3, 10, 500]] = [1, 98, 1]
    assert [ST.percentile_bin(hist, p) for p in (1, 2, 99, 100)] == [3, 10, 10, 500]
    assert [R.pct_bin(hist, p) for p in (1, 2, 99, 100)] == [3, 10, 10, 500]
    hist[3] = 2 ** 40  # (p m + 99) // 100 in integers beyond 2^32
    assert ST.percentile_bin(hist, 99) == R.pct_bin(hist, 99) == 3
    assert ST.percentile_bin(np.zeros(8, np.uint64), 1) == R.pct_bin(np.zeros(8, np.uint64), 1) == 0


def fallback_images():
    white = np.full((80, 80, 3), 255, np.uint8)
    one = np.full((80, 80, 3), (120, 40, 130), np.uint8)
    ten = white.copy()
    ten[5, 10:20] = R.synthetic_he(1, 10, seed=4, glass=0.0)[0]
    return {"white": (white, 0), "one colour": (one, 6400), "ten stained": (ten, None)}


@pytest.mark.parametrize("name", ["white", "one colour", "ten stained"])
def test_nothing_to_fit_returns_the_input(name):
    image, n = fallback_images()[name]
    before = image.copy()
    out, info = ST.normalize(image, kernels=REF)
    assert out is image and np.array_equal(image, before)
    assert info["applied"] is False and isinstance(info["reason"], str) and info["reason"] and info["T"] is None
    ref_out, ref = R.normalize_int(image)
    assert ref_out is image and not ref["applied"]
    if name == "white":
        assert "0 stained" in info["reason"]
    elif name == "one colour":
        assert "eigenvalue" in info["reason"] and ref["reason"] == "second eigenvalue"
        with pytest.raises(ST.StainFitError, match="eigenvalue"):
            ST.fit(image, kernels=REF)
    else:
        assert 1 <= ref["n_stained"] <= 10 and f"{ref['n_stained']} stained" in info["reason"]
    with pytest.raises(TypeError, match="StainFit"):
        ST.normalize(image, "macenko", kernels=REF)


def test_a_transform_beyond_the_integer_range_is_a_fallback(images):
    tiny = ST.StainFit(ST.MACENKO_TARGET.HE, [500.0, 500.0])  # a target 200 times as strong as the image
    out, info = ST.normalize(images[0], tiny, kernels=REF)
    assert out is images[0] and info["applied"] is False and "64" in info["reason"] and np.abs(info["T"]).max() >= 64
    with pytest.raises(ValueError, match="64"):
        ST.apply(images[0], 64.0 * np.eye(3), kernels=REF)
    assert ST.transform_q(63.9999 * np.eye(3)).max() == 2 ** 20 - 2


def test_fit_json_round_trip(images):
    got = ST.fit(images[0], kernels=REF)
    back = ST.StainFit.from_json(json.loads(json.dumps(got.to_json())))
    assert np.array_equal(back.HE, got.HE) and np.array_equal(back.maxC, got.maxC)
    assert (back.n_stained, back.skipped) == (got.n_stained, got.skipped) and back.HE.dtype == np.float64
    assert ST.StainFit.from_json({"HE": R.TARGET_HE.tolist(), "maxC": [1.0, 2.0]}).n_stained == 0
    for bad in ({"HE": [[1, 2]], "maxC": [1, 1]}, {"HE": R.TARGET_HE.tolist(), "maxC": [1.0, 0.0]},
                {"HE": R.TARGET_HE.tolist(), "maxC": [1.0, float("nan")]}):
        with pytest.raises(ValueError, match="StainFit"):
            ST.StainFit.from_json(bad)


def test_fit_many_is_the_fit_of_the_summed_integer_outputs(images):
    a, b = images[0], R.synthetic_he(64, 128, seed=7, he=([0.55, 0.76, 0.35], [0.10, 0.95, 0.29]))
    many = ST.fit_many([a, b], kernels=REF)
    ref = R.fit_int([a, b])  # every pass's words summed over the images before its host step
    assert np.array_equal(many.HE, ref["HE"]) and np.array_equal(many.maxC, ref["maxC"])
    assert many.n_stained == ref["n_stained"] == ST.fit(a, kernels=REF).n_stained + ST.fit(b, kernels=REF).n_stained
    stacked = ST.fit(np.concatenate([a, b]), kernels=REF)  # the images count as one
    assert np.array_equal(stacked.HE, many.HE) and np.array_equal(stacked.maxC, many.maxC)
    assert not np.array_equal(many.HE, ST.fit(a, kernels=REF).HE)
    with pytest.raises(ValueError, match="no image"):
        ST.fit_many([], kernels=REF)


# ----------------------------------------------------------------------------- predict_image and the CLIs
class _Net:  # refused before the network is looked at
    training = False


def test_predict_image_refuses_a_target_that_is_no_fit():
    with pytest.raises(TypeError, match="StainFit"):
        PR.predict_image(_Net(), np.zeros((8, 8, 3), np.uint8), stain="macenko")
    with pytest.raises(ValueError, match="beta"):
        PR.predict_image(_Net(), np.zeros((8, 8, 3), np.uint8), stain=ST.MACENKO_TARGET, stain_beta=0.0)


BASE = ["--input", "x.png", "--model_dir", "ck"]


def test_cli_defaults_and_flags(tmp_path):
    a = PR.parse_arguments(BASE)
    assert (a.stain_norm, a.stain_target, a.stain_beta) == ("none", None, 0.15)
    a = PR.parse_arguments(BASE + ["--stain_norm", "macenko", "--stain_target", "t.json", "--stain_beta", "0.2"])
    assert (a.stain_norm, a.stain_target, a.stain_beta) == ("macenko", "t.json", 0.2)
    path = tmp_path / "t.json"
    path.write_text(json.dumps(ST.MACENKO_TARGET.to_json()))
    assert np.array_equal(ST.load_target(path).HE, R.TARGET_HE)
    f = ST.parse_arguments(["fit", "--input", "a.png", "b", "--out", "t.json"])
    assert (f.command, f.input, f.out, f.beta) == ("fit", ["a.png", "b"], "t.json", 0.15)


@pytest.mark.parametrize("flags", [["--stain_norm", "reinhard"], ["--stain_target", "t.json"],
                                   ["--stain_norm", "macenko", "--stain_beta", "0"],
                                   ["--stain_norm", "macenko", "--stain_beta", "6"], ["--stain_beta", "x"]])
def test_cli_refuses_bad_stain_flags(flags, capsys):
    with pytest.raises(SystemExit) as e:
        PR.parse_arguments(BASE + flags)
    assert e.value.code == 2 and "--stain" in capsys.readouterr().err
    for argv in (["fit", "--input", "a.png"], ["fit", "--input", "a.png", "--out", "t.json", "--beta", "0"], []):
        with pytest.raises(SystemExit):
            ST.parse_arguments(argv)
        capsys.readouterr()


def test_record_has_no_stain_key_without_stain():
    pred = PR.Prediction(None, None, None, None, np.array([40, 20, 4, 64]), PR.TilePlan(8, 8, 160, 56))
    assert pred.stain is None and pred.stain_image is None and "stain" not in PR.image_record("x.png", pred)
    pred.stain = {"applied": False, "reason": "0 stained pixels, fewer than 4096", "HE": None, "maxC": None,
                  "n_stained": None, "skipped": None, "T": None}
    rec = PR.image_record("x.png", pred)
    assert list(rec)[-1] == "stain" and rec["stain"] == pred.stain and rec["stain"] is not pred.stain


# ----------------------------------------------------------------------------- C ABI argument rules
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(K.lib_path()):
        B.build()
    return K.load()


A, A2 = 0x10000, 0x90000  # aligned addresses that are never dereferenced: every call below is refused on the host
B6 = (ctypes.c_int32 * 6)(16384, 0, 0, 0, 16384, 0)
T9 = (ctypes.c_int32 * 9)(16384, 0, 0, 0, 16384, 0, 0, 0, 16384)
T9_BIG = (ctypes.c_int32 * 9)(16384, 0, 0, 0, -(1 << 20), 0, 0, 0, 16384)
B6_BIG = (ctypes.c_int32 * 6)(16384, 0, 0, 0, 1 << 15, -(1 << 15))  # a row's sum of |B| at 2^16
addr = ctypes.addressof

ARGS = {
    "selunet_stain_moments": dict(img=A, H=37, W=53, od_q=A, beta_q=614, out=A, stream=None),
    "selunet_stain_angle_hist": dict(img=A, H=37, W=53, od_q=A, beta_q=614, B=addr(B6), dirs=A, out=A, stream=None),
    "selunet_stain_conc_hist": dict(img=A, H=37, W=53, od_q=A, beta_q=614, P_q=addr(B6), out=A, stream=None),
    "selunet_stain_apply": dict(img=A, H=37, W=53, od_q=A, T_q=addr(T9), exp_q=A, n_exp=5676, out=A2, stream=None),
}
REFUSALS = [(fn, bad, word) for fn in ARGS for bad, word in (
    (dict(img=None), "null"), (dict(od_q=None), "null"), (dict(H=0), "height and width"),
    (dict(W=65536), "height and width"), (dict(od_q=A + 2), "4-B aligned"))]
REFUSALS += [
    ("selunet_stain_moments", dict(out=None), "null"), ("selunet_stain_moments", dict(out=A + 4), "8-B aligned"),
    ("selunet_stain_angle_hist", dict(B=None), "null"), ("selunet_stain_angle_hist", dict(dirs=None), "null"),
    ("selunet_stain_angle_hist", dict(out=None), "null"), ("selunet_stain_angle_hist", dict(out=A + 4), "8-B aligned"),
    ("selunet_stain_angle_hist", dict(dirs=A + 1), "4-B aligned"), ("selunet_stain_angle_hist", dict(B=addr(B6_BIG)), "2^16"),
    ("selunet_stain_conc_hist", dict(P_q=None), "null"), ("selunet_stain_conc_hist", dict(out=None), "null"),
    ("selunet_stain_conc_hist", dict(out=A + 4), "8-B aligned"),
    ("selunet_stain_apply", dict(T_q=None), "null"), ("selunet_stain_apply", dict(exp_q=None), "null"),
    ("selunet_stain_apply", dict(out=None), "null"), ("selunet_stain_apply", dict(n_exp=0), "n_exp"),
    ("selunet_stain_apply", dict(n_exp=8193), "n_exp"), ("selunet_stain_apply", dict(T_q=addr(T9_BIG)), "2^20"),
    ("selunet_stain_apply", dict(out=A), "alias"), ("selunet_stain_apply", dict(out=A + 3 * 37 * 53 - 1), "alias"),
    ("selunet_stain_apply", dict(out=A - 3 * 37 * 53 + 1), "alias"),
]


@pytest.mark.parametrize("fn,bad,word", REFUSALS, ids=[f"{f[8:]}:{','.join(b)}:{i}" for i, (f, b, _) in enumerate(REFUSALS)])
def test_stain_calls_refuse_on_the_host(lib, fn, bad, word):
    args = dict(ARGS[fn])
    args.update(bad)
    assert getattr(lib, fn)(*args.values()) == 1
    assert fn[len("selunet_"):].encode() in lib.selunet_last_error() and word.encode() in lib.selunet_last_error()
    with pytest.raises(K.SelunetError, match=fn[len("selunet_"):]):
        K.call(fn, *args.values())


def test_bindings_match_the_argument_counts(lib):
    for fn, args in ARGS.items():
        assert len(K.SIGNATURES[fn][1]) == len(args), fn
    assert {f for f, _, _ in REFUSALS} == set(ARGS)
