"""selunet_act_amax: the exact range word of a BN+ReLU source, max over [m][c] of relu(y*scale_c + shift_c).

Truth: max(relu(fp64(y) * fp64(scale) + fp64(shift))) in numpy. Accepted: truth * (1 - 2^-20) <= word <=
truth * (1 + 2^-20). The kernel evaluates the loaders' fp32 expression, whose two rounding orders (one fma, or a
rounded product then a rounded sum) are each within 2^-24 * (|product| + |sum|) / |sum| of the fp64 value, so within
5 * 2^-24 < 2^-21 wherever |product| <= 4 |sum|. The data keeps the maximal element there: it is planted with a
product of 40 and a shift in [-1, 1] (sum in [39, 41]), and every other element is below 4 * 2.5 + 1 = 11 (y clipped
to +-4, |scale| <= 2.5, |shift| <= 1), so nothing else can take the maximum whichever way it rounds. An ulp-level
difference of the word is harmless to its consumers: the split operand scale keeps amax * 2^e < 2^14 against an fp16
maximum of 65504, two bits of headroom.

Shapes (m, c): less than a wave of vectors (1, 64); 128 vectors per pixel in one workgroup (7, 512); several
workgroups (1000, 128); the capped grid with its unrolled loop and 16 vectors of tail (65537, 64);
m*c = 4 * 999, a multiple of no power-of-two span above 4, on the form whose channel group moves per vector (333, 12:
3 vectors per pixel); and that form through the capped grid's unrolled loop (80660, 52: 13 vectors per pixel).
"""
import numpy as np
import pytest
import torch

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2.0 ** -20
SHAPES = [(1, 64), (7, 512), (1000, 128), (65537, 64), (333, 12), (80660, 52)]
PLANTED = 40.0


def positions(m, c):
    """Element 0, the last element, the ragged tail (inside the last two 16-byte vectors, not the last element),
    and one in the middle."""
    e = m * c
    return {"first": 0, "last": e - 1, "tail": e - 7, "middle": e // 2 + 1}


def make(m, c, seed, signed=False):
    """y, scale, shift (fp32 numpy) with every |relu(y*scale + shift)| < 11."""
    g = np.random.default_rng(seed)
    y = np.clip(g.standard_normal((m, c)), -4, 4).astype(np.float32)
    scale = (np.abs(g.standard_normal(c)).clip(0, 2) + 0.5).astype(np.float32)
    if signed:  # as tests/test_gpu_bn_sign.py: channels [0, 4) negative, [4, 8) exactly zero, a third of the rest negative
        scale[:4] *= -1
        scale[4:8] = 0
        scale[8:][g.random(c - 8) < 1 / 3] *= -1
    shift = g.uniform(-1, 1, c).astype(np.float32)
    return y, scale, shift


def plant(y, scale, pos):
    """Make element `pos` the maximum: its product is PLANTED (a negative y under a negative scale)."""
    ch = pos % y.shape[1]
    assert scale[ch] != 0
    y.reshape(-1)[pos] = np.float32(PLANTED / float(scale[ch]))


def truth(y, scale, shift):
    return float(np.maximum(y.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64), 0).max())


def run(y, scale, shift, word):
    """One selunet_act_amax call folding y into the device word; returns the tensors it keeps alive."""
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (y, scale, shift)]
    m, c = y.shape
    K.call("selunet_act_amax", K.ptr(t[0]), m, c, K.ptr(t[1]), K.ptr(t[2]), K.ptr(word), K.stream_ptr())
    return t


def check(word, want, what):
    got = float(word.cpu()[0])
    print(f"act_amax {what}: word {got!r} truth {want!r} rel {abs(got - want) / want if want else 0.0:.3e}")
    assert want * (1 - TOL) <= got <= want * (1 + TOL), (what, got, want)


@pytest.mark.parametrize("m,c", SHAPES)
@pytest.mark.parametrize("signed", [False, True])
def test_act_amax_positions(m, c, signed):
    """The maximum at element 0, at the last element, in the ragged tail and mid-tensor; signed: scales of both
    signs and exactly zero (the planted element of a negative-scale channel has a negative y)."""
    y0, scale, shift = make(m, c, 100 + m % 97 + c, signed)
    if signed:
        assert (scale < 0).mean() >= 0.25 and (scale == 0).sum() == 4 and (scale > 0).any()
    for where, pos in positions(m, c).items():
        if scale[pos % c] == 0:  # (a zero-scale channel, [4, 8), cannot hold the maximum: four channels down)
            pos -= 4
        y = y0.copy()
        plant(y, scale, pos)
        want = truth(y, scale, shift)
        assert PLANTED - 1 <= want <= PLANTED + 1 and truth(y0, scale, shift) < 11
        word = torch.zeros(1, device=DEV)
        keep = run(y, scale, shift, word)  # noqa: F841
        check(word, want, f"({m}, {c}) signed={signed} max at {where} ({pos})")


@pytest.mark.parametrize("m,c", [(7, 512), (333, 12), (65537, 64)])
@pytest.mark.parametrize("signed", [False, True])
def test_act_amax_all_negative_is_zero(m, c, signed):
    """Every pre-activation negative: relu gives 0 everywhere and the zeroed word stays exactly 0.0."""
    y, scale, shift = make(m, c, 7, signed)
    y = -(np.abs(y) + 0.1) * np.where(scale < 0, -1, 1).astype(np.float32)[None, :]
    shift = -np.abs(shift) - 0.01
    assert (y.astype(np.float64) * scale + shift < 0).all()
    word = torch.zeros(1, device=DEV)
    keep = run(y.astype(np.float32), scale, shift.astype(np.float32), word)  # noqa: F841
    assert float(word.cpu()[0]) == 0.0 and not np.signbit(word.cpu().numpy()[0])


@pytest.mark.parametrize("m,c", [(1000, 128), (333, 12)])
def test_act_amax_preset_word(m, c):
    """A word already above the data's maximum is untouched (bit for bit); a smaller one is raised to it."""
    y, scale, shift = make(m, c, 21, signed=True)
    plant(y, scale, positions(m, c)["middle"] if scale[(m * c // 2 + 1) % c] != 0 else 0)
    want = truth(y, scale, shift)
    big = torch.full((1,), 1.0e6, device=DEV)
    keep = run(y, scale, shift, big)  # noqa: F841
    assert float(big.cpu()[0]) == 1.0e6
    small = torch.full((1,), 1.0, device=DEV)
    keep2 = run(y, scale, shift, small)  # noqa: F841
    check(small, want, f"({m}, {c}) raised from 1.0")


def test_act_amax_two_tensors_one_word():
    """Two calls fold two tensors (different shapes) into one word: the max of both, in either order."""
    ya, sa, ha = make(1000, 128, 31)
    yb, sb, hb = make(333, 12, 32, signed=True)
    plant(ya, sa, 12345)
    yb.reshape(-1)[13] = np.float32(2 * PLANTED / float(sb[13 % 12]))  # the larger of the two: a product of 80
    ta, tb = truth(ya, sa, ha), truth(yb, sb, hb)
    assert tb > 1.5 * ta > 50
    for first, second in (((ya, sa, ha), (yb, sb, hb)), ((yb, sb, hb), (ya, sa, ha))):
        word = torch.zeros(1, device=DEV)
        keep = run(*first, word), run(*second, word)  # noqa: F841
        check(word, max(ta, tb), "two tensors")


def test_act_amax_rejects_bad_arguments():
    y = torch.zeros(4, 6, device=DEV)
    s = torch.ones(6, device=DEV)
    w = torch.zeros(1, device=DEV)
    with pytest.raises(K.SelunetError):  # c not a multiple of 4
        K.call("selunet_act_amax", K.ptr(y), 4, 6, K.ptr(s), K.ptr(s), K.ptr(w), K.stream_ptr())
    with pytest.raises(K.SelunetError):
        K.call("selunet_act_amax", K.ptr(y), 0, 8, K.ptr(s), K.ptr(s), K.ptr(w), K.stream_ptr())
