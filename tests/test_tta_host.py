"""Flip / D4 test-time augmentation without a GPU: the eight maps of tests/_tta_ref.py form
the group D4, the argument rules of the four new entry points (host-side, before any launch), and — on the
CPU oracle — what the feature is for: the D4 ensemble's planes do not depend on the orientation the image
arrives in (to the rounding of a reordered sum), while the plain prediction's visibly do."""
import itertools

import numpy as np
import pytest

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import build as B
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR
from tests import _predict_ref as R
from tests import _tta_ref as TR

F32 = np.float32


# ----------------------------------------------------------------------------- the maps
def test_inverse_undoes_every_map_on_a_non_square_array():
    p = np.arange(5 * 7).reshape(5, 7)
    rgb = np.arange(5 * 7 * 3).reshape(5, 7, 3)
    for k in range(8):
        assert TR.T(k, p).shape == ((7, 5) if k & 4 else (5, 7))
        assert np.array_equal(TR.T_inv(k, TR.T(k, p)), p) and np.array_equal(TR.T(k, TR.T_inv(k, p.T if k & 4 else p)),
                                                                              p.T if k & 4 else p)
        assert np.array_equal(TR.T_inv(k, TR.T(k, rgb)), rgb)
        assert np.array_equal(TR.T(k, rgb)[..., 1], TR.T(k, rgb[..., 1]))  # the channels ride along


def test_the_eight_maps_are_distinct_and_closed_under_composition():
    p = np.arange(6 * 6).reshape(6, 6)  # square, so that every composition is defined on it
    images = [TR.T(k, p).tobytes() for k in range(8)]
    assert len(set(images)) == 8
    for a, b in itertools.product(range(8), repeat=2):
        assert TR.T(a, TR.T(b, p)).tobytes() in images, (a, b)
    assert TR.MEMBERS == {"flips": 4, "d4": 8} and PR.TTA_MEMBERS == {"none": 1, "flips": 4, "d4": 8}


def test_reduction_order_votes_and_mask_rule():
    rng = np.random.Generator(np.random.PCG64(5))
    m = [rng.normal(0, 3, (3, 5)).astype(F32) for _ in range(8)]
    A = ((m[0] + m[1]) + m[2]) + m[3]
    Bt = (((m[4].T + m[5].T) + m[6].T) + m[7].T).T  # accumulated in the transposed orientation
    assert np.array_equal(TR.reduce_members(m[:4]), A * F32(0.25))
    assert np.array_equal(TR.reduce_members(m), (A + Bt) * F32(0.125))
    nan = np.array([[np.nan, 1.0, -1.0]], F32)
    assert TR.votes_of([nan, nan], 0.0).tolist() == [[0, 2, 0]]
    assert TR.mask_of(nan, None, 0.0, 0.0).tolist() == [[0, 255, 0]]
    assert TR.mask_of(nan, nan[:, ::-1].copy(), 0.0, 0.0).tolist() == [[127, 255, 127]]


# ----------------------------------------------------------------------------- C ABI argument rules
@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(K.lib_path()):
        B.build()
    return K.load()


A = 0x10000  # a 16-B aligned address that is never dereferenced: every call below is refused on the host

ARGS = {
    "selunet_tile_gather_flip": dict(img=A, H=37, W=53, origins=A, n=3, th=16, tw=16, mode=0, flip=3, x=A, stream=None),
    "selunet_image_transpose": dict(src=A, H=37, W=53, dst=A + 16, stream=None),
    "selunet_tta_accumulate": dict(out=A, sel=A, origins=A, n=9, th=24, tw=24, halo=8, flip=1, first=0, H=37, W=53,
                                   ws=56, t_out=0.0, t_sel=0.0, sum_out=A, sum_sel=A, votes=A, sel_votes=A, stream=None),
    "selunet_tta_finalize": dict(a_out=A, a_sel=A, a_votes=A, a_sel_votes=A, b_out=A, b_sel=A, b_votes=A,
                                 b_sel_votes=A, members=8, H=37, W=53, wa=56, hb=40, t_out=0.0, t_sel=0.0,
                                 logit_plane=A, sel_plane=A, mask=A, prob8=A, votes=A, sel_votes=A, counts=A,
                                 stream=None),
}
NO_B = dict(b_out=None, b_sel=None, b_votes=None, b_sel_votes=None)
# (call, the arguments that differ from ARGS, a word of the message)
REFUSALS = [
    ("selunet_tile_gather_flip", dict(img=None), "null"), ("selunet_tile_gather_flip", dict(x=None), "null"),
    ("selunet_tile_gather_flip", dict(origins=None), "null origins"), ("selunet_tile_gather_flip", dict(n=0), "n must"),
    ("selunet_tile_gather_flip", dict(H=0), "height and width"), ("selunet_tile_gather_flip", dict(W=65536), "height and width"),
    ("selunet_tile_gather_flip", dict(th=20), "multiples of 8"), ("selunet_tile_gather_flip", dict(tw=4), "multiples of 8"),
    ("selunet_tile_gather_flip", dict(mode=3), "mode"), ("selunet_tile_gather_flip", dict(flip=4), "flip"),
    ("selunet_tile_gather_flip", dict(flip=-1), "flip"), ("selunet_tile_gather_flip", dict(x=A + 8), "16-B aligned"),
    ("selunet_image_transpose", dict(src=None), "null"), ("selunet_image_transpose", dict(dst=None), "null"),
    ("selunet_image_transpose", dict(dst=A), "in place"), ("selunet_image_transpose", dict(H=0), "height and width"),
    ("selunet_image_transpose", dict(W=65536), "height and width"),
    ("selunet_tta_accumulate", dict(out=None), "null"), ("selunet_tta_accumulate", dict(sum_out=None), "null"),
    ("selunet_tta_accumulate", dict(votes=None), "null"), ("selunet_tta_accumulate", dict(sel=None), "all be given"),
    ("selunet_tta_accumulate", dict(sum_sel=None), "all be given"), ("selunet_tta_accumulate", dict(sel_votes=None), "all be given"),
    ("selunet_tta_accumulate", dict(origins=None), "null origins"), ("selunet_tta_accumulate", dict(n=0), "n must"),
    ("selunet_tta_accumulate", dict(H=65536), "height and width"), ("selunet_tta_accumulate", dict(th=28), "multiples of 8"),
    ("selunet_tta_accumulate", dict(halo=4), "halo"), ("selunet_tta_accumulate", dict(halo=16), "halo"),
    ("selunet_tta_accumulate", dict(flip=4), "flip"), ("selunet_tta_accumulate", dict(flip=-1), "flip"),
    ("selunet_tta_accumulate", dict(first=2), "first"), ("selunet_tta_accumulate", dict(ws=48), "row stride"),
    ("selunet_tta_accumulate", dict(ws=60), "row stride"), ("selunet_tta_accumulate", dict(out=A + 4), "16-B aligned"),
    ("selunet_tta_accumulate", dict(sum_sel=A + 8), "16-B aligned"), ("selunet_tta_accumulate", dict(votes=A + 8), "16-B aligned"),
    ("selunet_tta_finalize", dict(members=1), "members"), ("selunet_tta_finalize", dict(members=6), "members"),
    ("selunet_tta_finalize", dict(a_out=None), "null"), ("selunet_tta_finalize", dict(a_votes=None), "null"),
    ("selunet_tta_finalize", dict(logit_plane=None), "null"), ("selunet_tta_finalize", dict(mask=None), "null"),
    ("selunet_tta_finalize", dict(votes=None), "null"), ("selunet_tta_finalize", dict(counts=None), "null"),
    ("selunet_tta_finalize", dict(a_sel=None), "all be given"), ("selunet_tta_finalize", dict(sel_plane=None), "all be given"),
    ("selunet_tta_finalize", dict(sel_votes=None), "all be given"), ("selunet_tta_finalize", dict(b_out=None), "8 members"),
    ("selunet_tta_finalize", dict(b_sel=None), "8 members"), ("selunet_tta_finalize", dict(members=4), "4 members"),
    ("selunet_tta_finalize", dict(members=4, **dict(NO_B, b_votes=A)), "4 members"),
    ("selunet_tta_finalize", dict(H=0), "height and width"), ("selunet_tta_finalize", dict(wa=48), "row stride wa"),
    ("selunet_tta_finalize", dict(wa=60), "row stride wa"), ("selunet_tta_finalize", dict(hb=32), "row stride hb"),
    ("selunet_tta_finalize", dict(hb=44), "row stride hb"), ("selunet_tta_finalize", dict(a_out=A + 4), "16-B aligned"),
    ("selunet_tta_finalize", dict(b_votes=A + 8), "16-B aligned"), ("selunet_tta_finalize", dict(prob8=A + 1), "16-B aligned"),
    ("selunet_tta_finalize", dict(counts=A + 4), "8-B aligned"),
]


def refused(fn, bad, word):
    """The call with ARGS[fn] changed by `bad` is refused on the host with `word` in its message."""
    args = dict(ARGS[fn])
    args.update(bad)
    assert K.load()
    with pytest.raises(K.SelunetError, match=fn[len("selunet_"):]) as e:
        K.call(fn, *args.values())
    assert word in str(e.value), (fn, bad, str(e.value))


@pytest.mark.parametrize("fn,bad,word", REFUSALS, ids=[f"{f[8:]}:{','.join(f'{k}={v}' for k, v in b.items())}"[:60]
                                                       for f, b, _ in REFUSALS])
def test_tta_calls_refuse_on_the_host(lib, fn, bad, word):
    refused(fn, bad, word)


def test_bindings_match_the_argument_counts(lib):
    for fn, args in ARGS.items():
        assert len(K.SIGNATURES[fn][1]) == len(args), fn
    # a 4-member finalize without the transposed class, and a head-less one, pass the same rules: the first
    # refusal they meet is a later one
    refused("selunet_tta_finalize", dict(NO_B, members=4, wa=48), "row stride wa")
    refused("selunet_tta_finalize", dict(a_sel=None, a_sel_votes=None, sel_plane=None, sel_votes=None, b_sel=None,
                                         b_sel_votes=None, wa=48), "row stride wa")
    refused("selunet_tta_accumulate", dict(sel=None, sum_sel=None, sel_votes=None, ws=48), "row stride")


def test_predict_image_refuses_an_unknown_tta():
    class Net:  # refused before the network is looked at
        training = False
    with pytest.raises(ValueError, match="tta"):
        PR.predict_image(Net(), np.zeros((8, 8, 3), np.uint8), tta="rot90")


# ----------------------------------------------------------------------------- the oracle's fact
H_O, W_O, TILE, HALO = 37, 70, 160, 56


@pytest.fixture(scope="module")
def oracle_case():
    """Tiled oracle predictions (tests/_predict_ref.py) of the eight orientations of a 37 x 70 image: a 1 x 2
    grid of 160 x 160 tiles, 2 x 1 transposed — 16 forwards, kept by image so that the ensemble of a
    transformed image, whose members are the same eight images, costs none."""
    forward = R.oracle_forward(*R.calibrated_state())
    done = {}

    def plain(image):
        key = (image.shape, image.tobytes())
        if key not in done:
            out, sel = R.predict_ref(forward, image, TILE, HALO)
            done[key] = (out[:image.shape[0], :image.shape[1]], sel[:image.shape[0], :image.shape[1]])
        return done[key]

    return {"plain": plain, "image": R.sample_image(H_O, W_O), "done": done}


def test_d4_ensemble_does_not_depend_on_the_orientation_of_the_image(oracle_case):
    """The D4 planes of T_5(image), mapped back, against those of the image: the same eight member planes summed
    in another order. Reordering a sum of 8 fp32 terms moves it by at most 7 * 2^-24 * sum |m_k|, i.e. the mean
    by 4.2e-7 * max |m_k|: bound 1e-6 * max |member logit|. The plain prediction misses that bound, so the
    comparison is not vacuous."""
    c = oracle_case
    t = MT.logit_threshold("eval", 0.5)
    image, turned = c["image"], np.ascontiguousarray(TR.T(5, c["image"]))
    ref = TR.tta_ref(c["plain"], image, 8, t, t)
    assert len(c["done"]) == 8 and R.grid_of(H_O, W_O, TILE, HALO)[1] == (1, 2)
    got = TR.tta_ref(c["plain"], turned, 8, t, t)
    assert len(c["done"]) == 8  # the turned image's members are the same eight images
    assert got["logit"].shape == (W_O, H_O) and ref["logit"].shape == (H_O, W_O)
    for head, i in (("logit", 0), ("selection", 1)):
        top = max(float(np.abs(m[i]).max()) for m in ref["members"])
        bound = 1e-6 * top
        e_tta = float(np.abs(TR.T_inv(5, got[head]) - ref[head]).max())
        e_plain = float(np.abs(TR.T_inv(5, c["plain"](turned)[i]) - c["plain"](image)[i]).max())
        print(f"{head}: max |member| {top:.4f}, bound {bound:.3e}; d4 of T_5(image) mapped back vs d4 of the image "
              f"{e_tta:.3e}; plain {e_plain:.3e}")
        assert e_tta <= bound
        assert e_plain > bound
    assert np.ptp(ref["logit"]) > 0.1 and np.ptp(ref["selection"]) > 0.1  # the heads spread
    assert ref["votes"].dtype == np.uint8 and ref["votes"].max() <= 8
    assert np.array_equal(TR.T_inv(5, got["votes"]), ref["votes"])  # votes are counts: no rounding to reorder
