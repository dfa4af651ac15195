"""Flip / D4 test-time augmentation of whole-image prediction on the GPU: the four kernels
against numpy and the existing kernels, bit for bit; `predict_image(..., tta=)` against the pinned reduction
(tests/_tta_ref.py) of plain `predict_image` calls on the transformed images; and the predict CLI's files."""
import json

import numpy as np
import pytest
import torch

import selectivenet_for_semantic_segmentation_binary_amd as S
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR
from tests import _golden as G
from tests import _predict_ref as R
from tests import _tta_ref as TR
from tests.test_tta_host import REFUSALS, refused

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
T_OUT = F32(MT.logit_threshold("eval", 0.5))
T_SEL = F32(MT.logit_threshold("eval", 0.7))


def dev(a):
    return torch.tensor(np.array(a, order="C"), device=DEV)  # a copy: a flipped axis of length 1 keeps its stride


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """Bit-equal fp32 arrays, a NaN matching any NaN (the sign and payload of a NaN that an addition makes, as
    inf + -inf, are the adder's choice)."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


with np.errstate(invalid="ignore"):
    _T = np.array([T_OUT, T_SEL], F32)
    EDGE = np.concatenate([_T, np.nextafter(_T, F32(-np.inf)), np.nextafter(_T, F32(np.inf)),
                           np.array([0, -0.0, np.inf, -np.inf, np.nan, 40, -40, 20.5, -20.5, 100, -100], F32)]).astype(F32)


# ----------------------------------------------------------------------------- flipped gather
# 16 x 16 tiles: negative, several folds in both directions, interior (the 12-B load at every byte alignment,
# forwards and reversed), one whose last group ends on the image's last pixel, one across and one past the edge
GATHER_ORIGINS = np.array([(-8, -8), (-40, 60), (8, 16), (13, 21), (21, 37), (24, 40), (-100, -131)], np.int32)


@pytest.mark.parametrize("input_type", ["RGB", "GH", "H_RGB"])
@pytest.mark.parametrize("H,W", [(37, 53), (1, 9)])
def test_flipped_gather_equals_gather_of_the_flipped_image(H, W, input_type):
    rng = np.random.Generator(np.random.PCG64(H * 100 + W))
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    origins = dev(GATHER_ORIGINS)
    seen = set()
    for k in range(4):
        want = PR.tile_gather(dev(TR.T(k, image)), origins, 16, 16, input_type).cpu().numpy()
        got = PR.tile_gather_flip(dev(image), origins, 16, 16, input_type, k)
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), k
        seen.add(want.tobytes())
    assert len(seen) == (4 if H > 1 else 2)  # the flips differ: the equality is not of one image with itself
    buf = torch.full((8,) + want.shape[1:], 7.0, device=DEV)  # into a slice of a larger buffer
    PR.tile_gather_flip(dev(image), origins[:2], 16, 16, input_type, 3, out=buf[:2])
    assert np.array_equal(bits(buf[:2].cpu().numpy()), bits(want[:2])) and (buf[2:] == 7.0).all()


# ----------------------------------------------------------------------------- image transpose
@pytest.mark.parametrize("H,W", [(1, 9), (37, 53), (64, 64), (33, 130)])
def test_image_transpose_equals_numpy(H, W):
    rng = np.random.Generator(np.random.PCG64(H * 1000 + W))
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    got = PR.image_transpose(dev(image))
    assert got.shape == (W, H, 3) and got.dtype == torch.uint8 and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), image.transpose(1, 0, 2))
    assert np.array_equal(got.cpu().numpy(), TR.T(4, image))


# ----------------------------------------------------------------------------- accumulate
H_A, W_A, TILE_A, HALO_A = 37, 53, 24, 8
ZERO_AT = (21, 30)


@pytest.fixture(scope="module")
def acc_case():
    """Four members of 5 x 7 tiles of 24 x 24 (cores of 8 x 8, canvas 40 x 56) over a 37 x 53 image; scores
    ~ N(0, 3) with, along the first rows of every core, each threshold, its two fp32 neighbours, +-0, +-inf, NaN
    and saturated values, shifted from member to member so that they also meet each other in the sums."""
    core, grid, origins = R.grid_of(H_A, W_A, TILE_A, HALO_A)
    origins = origins.astype(np.int32)
    n = len(origins)
    assert grid == (5, 7) and core == 8
    rng = np.random.Generator(np.random.PCG64(31))
    tiles, planes = [], []
    for f in range(4):
        out = rng.normal(0, 3, (n, TILE_A, TILE_A)).astype(F32)
        sel = rng.normal(0, 3, (n, TILE_A, TILE_A)).astype(F32)
        for t in range(n):
            e = np.roll(EDGE, -(8 * t + 3 * f))
            out[t, HALO_A, HALO_A:HALO_A + 8] = e[:8]
            sel[t, HALO_A + 1, HALO_A:HALO_A + 8] = e[8:16]
            out[t, HALO_A + 2, HALO_A:HALO_A + 8] = e[:8]
            sel[t, HALO_A + 2, HALO_A:HALO_A + 8] = e[7::-1]
        # image pixel ZERO_AT holds -0 in every member (at T_f of it in member f's canvas): the sum is -0
        cy, cx = (H_A - 1 - ZERO_AT[0] if f & 2 else ZERO_AT[0]), (W_A - 1 - ZERO_AT[1] if f & 1 else ZERO_AT[1])
        assert cy % 8 > 2  # not one of the rows above
        for v in (out, sel):
            v[(cy // 8) * 7 + cx // 8, HALO_A + cy % 8, HALO_A + cx % 8] = -0.0
        tiles.append((out, sel))
        # the member's canvas, cut to its image, mapped back to the image's orientation
        planes.append(tuple(np.ascontiguousarray(TR.T_inv(f, R.stitch(v, origins, HALO_A, 40, 56)[:H_A, :W_A]))
                            for v in (out, sel)))
    with np.errstate(invalid="ignore", over="ignore"):
        sums = []
        for i in range(2):
            a = planes[0][i]
            for f in range(1, 4):
                a = a + planes[f][i]
            sums.append(a)
    return {"origins": origins, "tiles": tiles, "sum_out": sums[0], "sum_sel": sums[1],
            "votes": TR.votes_of([p[0] for p in planes], T_OUT), "sel_votes": TR.votes_of([p[1] for p in planes], T_SEL)}


def run_accumulate(c, parts=None, selective=True, rows=H_A + 3, ws=56):
    """The planes [rows, ws], filled with -777 / 77 beforehand, after the four members in the calls `parts`."""
    n = len(c["origins"])
    s_out = torch.full((rows, ws), -777.0, device=DEV)
    s_sel = torch.full((rows, ws), -777.0, device=DEV) if selective else None
    v_out = torch.full((rows, ws), 77, dtype=torch.uint8, device=DEV)
    v_sel = torch.full((rows, ws), 77, dtype=torch.uint8, device=DEV) if selective else None
    for f in range(4):
        for part in parts or [list(range(n))]:
            oh = np.ascontiguousarray(c["origins"][part])
            PR.tta_accumulate(dev(c["tiles"][f][0][part]), dev(c["tiles"][f][1][part]) if selective else None, oh, dev(oh),
                              HALO_A, f, f == 0, H_A, W_A, 40, 56, float(T_OUT), float(T_SEL), s_out, s_sel, v_out, v_sel)
    return {"sum_out": s_out.cpu().numpy(), "sum_sel": None if s_sel is None else s_sel.cpu().numpy(),
            "votes": v_out.cpu().numpy(), "sel_votes": None if v_sel is None else v_sel.cpu().numpy()}


def check_accumulated(got, c, selective=True):
    for k in ("sum_out", "sum_sel") if selective else ("sum_out",):
        assert same(got[k][:H_A, :W_A], c[k]), k
        outside = got[k].copy()
        outside[:H_A, :W_A] = -777.0
        assert (outside == -777.0).all(), k  # words outside the image: as they were
    for k in ("votes", "sel_votes") if selective else ("votes",):
        assert np.array_equal(got[k][:H_A, :W_A], c[k]), k
        outside = got[k].copy()
        outside[:H_A, :W_A] = 77
        assert (outside == 77).all(), k


def test_accumulate_sums_and_votes_equal_numpy(acc_case):
    c = acc_case
    assert np.isnan(c["sum_out"]).any() and np.isinf(c["sum_out"]).any() and set(np.unique(c["votes"])) == {0, 1, 2, 3, 4}
    assert bits(c["sum_out"])[ZERO_AT] == bits(c["sum_sel"])[ZERO_AT] == 0x80000000  # -0 + -0 + -0 + -0, not +0 + ...
    check_accumulated(run_accumulate(c), c)


def test_accumulate_two_calls_equal_one(acc_case):
    c = acc_case
    n = len(c["origins"])
    check_accumulated(run_accumulate(c, parts=[list(range(0, 17)), list(range(17, n))]), c)
    check_accumulated(run_accumulate(c, parts=[list(range(n - 1, 4, -1)), [0, 1, 2, 3, 4]]), c)  # any order of tiles


def test_accumulate_without_a_selection_head_and_with_wider_planes(acc_case):
    c = acc_case
    got = run_accumulate(c, selective=False)
    assert got["sum_sel"] is None and got["sel_votes"] is None
    check_accumulated(got, c, selective=False)
    check_accumulated(run_accumulate(c, ws=72, rows=41), c)


def test_accumulate_wrapper_refuses_cores_outside_the_canvas(acc_case):
    c = acc_case
    z = lambda dt: torch.zeros(40, 56, dtype=dt, device=DEV)  # noqa: E731
    for y0, x0 in ((-16, -8), (-8, -16), (32, -8), (-8, 48), (-8, -4)):
        oh = np.array([[y0, x0]], np.int32)
        with pytest.raises(K.SelunetError, match="core"):
            PR.tta_accumulate(dev(c["tiles"][0][0][:1]), None, oh, dev(oh), HALO_A, 0, True, H_A, W_A, 40, 56, 0.0, 0.0,
                              z(torch.float32), None, z(torch.uint8), None)


# ----------------------------------------------------------------------------- finalize
def finalize_case(H, W, members, seed):
    """Sums and votes of the two classes, [H, wa] and [W, hb] (padding zero, as predict_image keeps it), whose
    means land on each threshold and its fp32 neighbours (4 t and 8 t are exact in fp32), on +-0, +-inf, NaN
    and saturated values, among N(0, 3 K) noise."""
    rng = np.random.Generator(np.random.PCG64(seed))
    wa, hb = -(-W // 8) * 8, -(-H // 8) * 8

    def planes(h, w, ws):
        s = [np.zeros((h, ws), F32) for _ in range(2)]
        v = [np.zeros((h, ws), np.uint8) for _ in range(2)]
        for i in range(2):
            s[i][:, :w] = rng.normal(0, 12, (h, w)).astype(F32)
            v[i][:, :w] = rng.integers(0, 5, (h, w), dtype=np.uint8)
        return s, v

    (a_out, a_sel), (a_vo, a_vs) = planes(H, W, wa)
    (b_out, b_sel), (b_vo, b_vs) = planes(W, H, hb)
    k = min(len(EDGE), W)
    for y in range(0, H, 5):
        e = np.roll(EDGE, -y)[:k]
        if members == 4:
            a_out[y, :k], a_sel[(y + 1) % H, :k] = e * F32(4), e * F32(4)
        else:  # the mean is (A + B^T) / 8: half of 8 t from either class, and all of it from one
            a_out[y, :k], b_out[:k, y] = e * F32(4), e * F32(4)
            a_sel[(y + 1) % H, :k], b_sel[:k, (y + 1) % H] = e * F32(8), 0
    a, b = (a_out, a_sel, a_vo, a_vs), (b_out, b_sel, b_vo, b_vs)
    with np.errstate(invalid="ignore", over="ignore"):
        if members == 4:
            mo, ms, vo, vs = a_out * F32(0.25), a_sel * F32(0.25), a_vo, a_vs
        else:
            mo, ms = (a_out[:, :W] + b_out[:, :H].T) * F32(0.125), (a_sel[:, :W] + b_sel[:, :H].T) * F32(0.125)
            vo, vs = a_vo[:, :W] + b_vo[:, :H].T, a_vs[:, :W] + b_vs[:, :H].T
    want = {"logit": mo[:, :W], "selection": ms[:, :W], "votes": vo[:, :W], "sel_votes": vs[:, :W]}
    return a, (b if members == 8 else None), want


@pytest.mark.parametrize("selective", [True, False])
@pytest.mark.parametrize("H,W", [(37, 53), (33, 130)])
@pytest.mark.parametrize("members", [4, 8])
def test_finalize_means_mask_votes_and_counts_equal_numpy(members, H, W, selective):
    a, b, want = finalize_case(H, W, members, seed=H + members)
    pick = (lambda g: None if g is None else tuple(dev(t) if selective or i in (0, 2) else None for i, t in enumerate(g)))  # noqa: E731
    planes, counts = PR.tta_finalize(pick(a), pick(b), members, H, W, float(T_OUT), float(T_SEL))
    logit, selection, mask, prob8, votes, sel_votes = [None if t is None else t.cpu().numpy()[:, :W] for t in planes]
    assert logit.shape == (H, W) and (selection is None) == (not selective) == (sel_votes is None)
    assert same(logit, want["logit"]) and np.array_equal(votes, want["votes"])
    for t in _T:  # the means land on the thresholds and on both neighbours
        for v in (t, np.nextafter(t, F32(-np.inf)), np.nextafter(t, F32(np.inf))):
            assert (bits(want["logit"]) == bits(np.array([v], F32))[0]).any(), v
    if selective:
        assert same(selection, want["selection"]) and np.array_equal(sel_votes, want["sel_votes"])
    want_mask = TR.mask_of(want["logit"], want["selection"] if selective else None, T_OUT, T_SEL)
    assert np.array_equal(mask, want_mask)
    got_counts = counts.cpu().numpy().tolist()
    assert got_counts == TR.counts_of(want_mask) and sum(got_counts[:3]) == got_counts[3] == H * W
    assert min(got_counts[:2]) > 0.1 * H * W and (got_counts[2] > 0.1 * H * W) == selective
    x = want["logit"].astype(np.float64)
    nan = np.isnan(x)
    with np.errstate(over="ignore"):
        level = np.floor(255.0 / (1.0 + np.exp(-x[~nan])) + 0.5)
    d = np.abs(prob8[~nan].astype(np.int64) - level.astype(np.int64))
    print(f"finalize K={members} {H} x {W}: prob8 differs from the fp64 level on {int((d != 0).sum())} of {d.size}, max {int(d.max())}")
    assert d.max() <= 1 and (prob8[nan] == 0).all() and nan.any()


def test_finalize_without_prob8():
    a, b, want = finalize_case(37, 53, 4, seed=1)
    planes, _ = PR.tta_finalize(tuple(dev(t) for t in a), None, 4, 37, 53, float(T_OUT), float(T_SEL), prob8=False)
    assert planes[3] is None and same(planes[0].cpu().numpy()[:, :53], want["logit"])


# ----------------------------------------------------------------------------- refusals
def test_each_entry_point_refuses_bad_arguments_with_its_message():
    for fn, bad, word in REFUSALS:
        refused(fn, bad, word)
    assert {f for f, _, _ in REFUSALS} == {"selunet_tile_gather_flip", "selunet_image_transpose",
                                           "selunet_tta_accumulate", "selunet_tta_finalize"}


# ----------------------------------------------------------------------------- whole path
H_I, W_I = 100, 140
KW = dict(tile=160, halo=56)


def make_net(state, **kw):
    net = S.UNet_B("RGB", selective=True, **kw)
    net.load_state_dict(state)
    return net.to(DEV).eval()


def plain_of(net, batch_size=4, **kw):
    """image -> (out, sel) numpy: today's predict_image."""
    def plain(image):
        p = PR.predict_image(net, image, batch_size=batch_size, **KW, **kw)
        return p.logit.cpu().numpy(), p.selection.cpu().numpy()
    return plain


def reference(mem, t_out, t_sel):
    """tests/_tta_ref.py's reduction, votes, mask and counts of the member planes `mem`."""
    outs, sels = [m[0] for m in mem], [m[1] for m in mem]
    ref = {"logit": TR.reduce_members(outs), "selection": TR.reduce_members(sels), "votes": TR.votes_of(outs, t_out),
           "sel_votes": TR.votes_of(sels, t_sel), "members": mem}
    ref["mask"] = TR.mask_of(ref["logit"], ref["selection"], t_out, t_sel)
    ref["counts"] = TR.counts_of(ref["mask"])
    return ref


@pytest.fixture(scope="module")
def whole():
    """The calibrated network of tests/test_gpu_predict.py, the 100 x 140 image, and the reference of either
    ensemble: tests/_tta_ref.py's reduction of eight plain predict_image calls in batches of 4 (computed once).
    The network's weights are not equivariant, so its members disagree and their mean selection lies below the
    default cut-off almost everywhere (the ensemble abstains). For all three mask classes to occur the cut-offs
    are set from the reference: sigmoid of the median of the reference's D4 mean plane, per head — half the
    pixels abstained, the rest split around the output's median."""
    state = R.state_dict_of(*R.calibrated_state())
    net = make_net(state)
    image = R.sample_image(H_I, W_I)
    mem = TR.member_planes(plain_of(net), image, 8)
    cuts = [float(1.0 / (1.0 + np.exp(-np.median(TR.reduce_members([m[i] for m in mem]).astype(np.float64)))))
            for i in range(2)]
    kw = dict(KW, cut_off=cuts[0], s_cut_off=cuts[1])
    t_out, t_sel = F32(MT.logit_threshold("eval", cuts[0])), F32(MT.logit_threshold("eval", cuts[1]))
    return {"state": state, "net": net, "image": image, "kw": kw, "t_out": t_out, "t_sel": t_sel,
            "d4": reference(mem, t_out, t_sel), "flips": reference(mem[:4], t_out, t_sel)}


def fields(pred):
    return {k: getattr(pred, k).cpu().numpy() for k in ("logit", "selection", "mask", "votes", "sel_votes", "prob8")}


def check_equal(pred, ref, members):
    got = fields(pred)
    assert pred.members == members and got["logit"].shape == (H_I, W_I)
    d = max(float(np.abs(got[k] - ref[k]).max()) for k in ("logit", "selection"))
    print(f"tta with {members} members vs the reduction of {members} plain calls: max |difference| {d}")
    assert d == 0.0 and same(got["logit"], ref["logit"]) and same(got["selection"], ref["selection"])
    for k in ("mask", "votes", "sel_votes"):
        assert got[k].dtype == np.uint8 and np.array_equal(got[k], ref[k]), k
    assert pred.counts.tolist() == ref["counts"] and int(pred.counts[3]) == H_I * W_I
    return got


@pytest.mark.parametrize("tta", ["flips", "d4"])
def test_tta_equals_the_reduction_of_plain_calls(whole, tta):
    w = whole
    members = TR.MEMBERS[tta]
    ref = w[tta]
    pred = PR.predict_image(w["net"], w["image"], batch_size=4, tta=tta, **w["kw"])
    got = check_equal(pred, ref, members)
    with np.errstate(over="ignore"):
        level = np.floor(255.0 / (1.0 + np.exp(-got["logit"].astype(np.float64))) + 0.5)
    assert np.abs(got["prob8"].astype(np.int64) - level.astype(np.int64)).max() <= 1
    # another batch size: the forwards see other batch shapes; the eval-forward bound
    other = PR.predict_image(w["net"], torch.from_numpy(w["image"]), batch_size=16, tta=tta, prob8=False, **w["kw"])
    e = max(G.max_rel(other.logit.cpu().numpy(), ref["logit"]), G.max_rel(other.selection.cpu().numpy(), ref["selection"]))
    print(f"tta={tta}, batches of 16 against the reference in batches of 4: max rel {e:.3e}")
    assert e < 1e-4 and other.prob8 is None and other.members == members


@pytest.mark.parametrize("tta", ["flips", "d4"])
def test_votes(whole, tta):
    w = whole
    members = TR.MEMBERS[tta]
    pred = PR.predict_image(w["net"], w["image"], batch_size=4, tta=tta, **w["kw"])
    votes, sel_votes = pred.votes.cpu().numpy(), pred.sel_votes.cpu().numpy()
    assert votes.shape == (H_I, W_I) and votes.max() <= members and sel_votes.max() <= members
    mem = w["d4"]["members"][:members]
    all_tumor = np.all([m[0] >= w["t_out"] for m in mem], axis=0)
    assert ((votes == members) <= all_tumor).all() and (votes == members).any()
    assert ((votes == 0) <= ~np.any([m[0] >= w["t_out"] for m in mem], axis=0)).all()
    assert min(pred.counts[:3]) > 0.02 * H_I * W_I  # the heads spread: all three classes occur
    u = pred.unanimous_fraction
    assert u == float(((votes == 0) | (votes == members)).mean()) and 0 < u < 1
    print(f"tta={tta}: counts {pred.counts.tolist()}, unanimous fraction {u:.4f}, votes histogram "
          f"{np.bincount(votes.ravel(), minlength=members + 1).tolist()}")


def test_d4_does_not_depend_on_the_orientation_of_the_image(whole):
    """tests/test_tta_host.py's fact on the device: bound 1e-6 * max |member logit| (a reordered sum of 8)."""
    w = whole
    turned = np.ascontiguousarray(TR.T(5, w["image"]))
    pred = PR.predict_image(w["net"], turned, batch_size=4, tta="d4", **w["kw"])
    plain = plain_of(w["net"])
    p_turned, p_image = plain(turned), plain(w["image"])
    for head, i, got in (("logit", 0, pred.logit), ("selection", 1, pred.selection)):
        top = max(float(np.abs(m[i]).max()) for m in w["d4"]["members"])
        e_tta = float(np.abs(TR.T_inv(5, got.cpu().numpy()) - w["d4"][head]).max())
        e_plain = float(np.abs(TR.T_inv(5, p_turned[i]) - p_image[i]).max())
        print(f"{head}: bound {1e-6 * top:.3e}; d4 of T_5(image) mapped back vs d4 of the image {e_tta:.3e}; plain {e_plain:.3e}")
        assert e_tta <= 1e-6 * top
        assert e_plain > 1e-6 * top
    assert np.array_equal(TR.T_inv(5, pred.votes.cpu().numpy()), w["d4"]["votes"])


def test_tta_none_is_the_plain_path(whole):
    w = whole
    a = PR.predict_image(w["net"], w["image"], batch_size=4, **KW)
    b = PR.predict_image(w["net"], w["image"], batch_size=4, tta="none", **KW)
    assert b.votes is None and b.sel_votes is None and b.members == 1 and b.unanimous_fraction is None
    assert a.votes is None and a.members == 1
    for k in ("logit", "selection"):
        assert np.array_equal(bits(getattr(a, k).cpu().numpy()), bits(getattr(b, k).cpu().numpy())), k
    assert torch.equal(a.mask, b.mask) and torch.equal(a.prob8, b.prob8) and a.counts.tolist() == b.counts.tolist()
    assert same(a.logit.cpu().numpy(), w["d4"]["members"][0][0])
    with pytest.raises(ValueError, match="tta"):
        PR.predict_image(w["net"], w["image"], tta="rot90", **KW)


def test_tta_on_the_split_path_and_in_bf16(whole):
    w = whole
    net = make_net(w["state"], fp32_eval_path="split")
    ref = reference(TR.member_planes(plain_of(net), w["image"], 4), w["t_out"], w["t_sel"])
    check_equal(PR.predict_image(net, w["image"], batch_size=4, tta="flips", **w["kw"]), ref, 4)
    net = make_net(w["state"], compute_dtype=torch.bfloat16)
    pred = PR.predict_image(net, w["image"], batch_size=4, tta="d4", **w["kw"])
    assert int(pred.counts[3]) == H_I * W_I and int(pred.counts[:3].sum()) == H_I * W_I and pred.members == 8
    print(f"bf16 d4: logits max rel {G.max_rel(pred.logit.cpu().numpy(), w['d4']['logit']):.3e} against fp32, "
          f"{(pred.mask.cpu().numpy() == w['d4']['mask']).mean():.4f} of the mask agrees")


def test_tta_without_a_selection_head(whole):
    net = S.UNet_B("RGB", selective=False)
    net.load_state_dict({k: v for k, v in whole["state"].items() if k in net.state_dict()})
    net = net.to(DEV).eval()
    pred = PR.predict_image(net, whole["image"], batch_size=4, tta="flips", **KW)
    assert pred.selection is None and pred.sel_votes is None and pred.votes is not None and pred.counts[2] == 0
    assert np.array_equal(pred.mask.cpu().numpy(), TR.mask_of(pred.logit.cpu().numpy(), None, T_OUT, T_OUT))


def test_predict_cli_with_tta_writes_votes(whole, tmp_path):
    from PIL import Image

    w = whole
    ck = tmp_path / "checkpoint"
    ck.mkdir()
    torch.save({"net": w["state"]}, ck / "model_epoch1.pth")
    src = tmp_path / "region.png"
    Image.fromarray(w["image"]).save(src)
    out = tmp_path / "out"
    doc = PR.predict_files(PR.parse_arguments([
        "--input", str(src), "--model_dir", str(ck), "--model_arch", "UNet_B", "--selective", "1", "--tile", "160",
        "--halo", "56", "--batch_size", "4", "--save_dir", str(out), "--tta", "flips", "--cut_off", repr(w["kw"]["cut_off"]),
        "--s_cut_off", repr(w["kw"]["s_cut_off"])]))
    on_disk = json.load(open(out / "predict.json"))
    assert on_disk == json.loads(json.dumps(doc)) and on_disk["tta"] == "flips"
    votes = np.array(Image.open(out / "region_votes.png"))
    assert votes.dtype == np.uint8 and np.array_equal(votes, w["flips"]["votes"].astype(np.int64) * 255 // 4)
    rec = on_disk["images"][0]
    assert rec["unanimous_fraction"] == float(((votes == 0) | (votes == 255)).mean())
    assert np.array_equal(np.array(Image.open(out / "region_mask.png")), w["flips"]["mask"])
    assert rec["counts"] == dict(zip(PR.COUNT_NAMES, w["flips"]["counts"]))
    # without --tta: no votes file, "tta": "none"
    plain = PR.predict_files(PR.parse_arguments([
        "--input", str(src), "--model_dir", str(ck), "--selective", "1", "--tile", "160", "--batch_size", "4",
        "--save_dir", str(tmp_path / "plain")]))
    assert plain["tta"] == "none" and plain["images"][0]["unanimous_fraction"] is None
    assert not (tmp_path / "plain" / "region_votes.png").exists()
