"""selunet_prep_batch_aug on the GPU against tests/_augment_ref.py, bit for bit.

The mirror decides, in numpy, which three bytes and which label byte of every output pixel enter the per-pixel
conversion. Each case is then held to it twice:

* exactly (`torch.equal` on the bits), for all three input types, against `data.prep_batch` — no flips — of the
  mirror's bytes: the conversion is the shared prep_pixel, whose promise is the same bits for the same bytes;
* against oracle/data_cpu.py's conversion of the mirror's bytes by the rules of tests/test_gpu_data.py: 'RGB' and
  the target bit for bit, 'GH' within 1e-6 / 1e-5 and 'H_RGB' within 1e-5 (logf against numpy's log).

The sizes are the smallest at which the kernel can go wrong: 8 x 8 (a quadrant edge on a 4-pixel group), 12 x 12
(inside one), 7 x 8 and 8 x 16 (odd and non-square), and 6 x 24 x 24 where three workgroups wrap."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import data_cpu as OD
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import data as D
from tests import _augment_ref as AR

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ["RGB", "GH", "H_RGB"]
CONV = {"RGB": lambda a: a, "GH": OD.rgb2gh, "H_RGB": OD.h_rgb}
TABLE = AR.glass_table()


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.tensor(a.view(np.int32) if a.dtype == np.uint32 else a, device=DEV)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def case(n, h, w, seed):
    """Random bytes with the extremes present; labels around the 255 -> 1 truncation."""
    rng = np.random.Generator(np.random.PCG64(seed))
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    img[:, 0, 0], img[:, -1, -1] = 0, 255
    lab = rng.choice(np.array([0, 1, 127, 254, 255], np.uint8), (n, h, w), p=[0.2, 0.1, 0.1, 0.1, 0.5])
    return rng, img, lab


def luts(rng, n):
    """A different random (not monotone) table per image and channel: a permutation of the bytes."""
    return np.stack([np.stack([rng.permutation(256).astype(np.uint8) for _ in range(3)]) for _ in range(n)])


def aug(img, lab, geom=None, glass=None, keys=None, lut=None, input_type="RGB", **kw):
    return D.prep_batch_aug(dev(img), dev(lab), dev(None if geom is None else np.asarray(geom, np.uint8)),
                            dev(None if glass is None else np.asarray(glass, np.uint8)),
                            dev(None if keys is None else np.asarray(keys, np.uint32)), dev(lut), input_type, **kw)


def check(img, lab, geom=None, glass=None, keys=None, lut=None, input_type="RGB"):
    """The call against the mirror (module docstring); returns (x, t, mirror image bytes, mirror label bytes)."""
    x, t = aug(img, lab, geom, glass, keys, lut, input_type)
    oi, ol = AR.augment_bytes(img, lab, geom, glass, keys, lut, TABLE)
    xp, tp = D.prep_batch(dev(oi), dev(ol), None, input_type)
    assert x.shape == xp.shape and t.shape == tp.shape and x.dtype == t.dtype == torch.float32
    assert torch.equal(bits(x), bits(xp)), "x differs from the conversion of the mirror's bytes"
    assert torch.equal(bits(t), bits(tp)), "target differs from the truncation of the mirror's label bytes"
    want = [OD.transform(CONV[input_type]((oi[i] / 255.0).astype(F32)), (ol[i] / 255.0).astype(np.uint8), 0)
            for i in range(len(oi))]
    xe, te = np.stack([a for a, _ in want]), np.stack([b for _, b in want])
    xg = x.cpu().numpy()
    assert torch.equal(t.cpu(), torch.from_numpy(te))
    if input_type == "RGB":
        assert torch.equal(bits(x.cpu()), bits(torch.from_numpy(xe)))
    elif input_type == "GH":
        assert np.abs(xg[:, 0] - xe[:, 0]).max() <= 1e-6 and np.abs(xg[:, 1] - xe[:, 1]).max() <= 1e-5
    else:
        assert np.abs(xg - xe).max() <= 1e-5
    return x, t, oi, ol


# ----------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("input_type", TYPES)
def test_flips_alone_are_todays_prep_batch(input_type):
    """geom in 0..3, no glass, no table: torch.equal to data.prep_batch with flips = geom (8 x 16 and odd 7 x 8)."""
    for n, h, w in ((5, 8, 16), (4, 7, 8)):
        _, img, lab = case(n, h, w, 11)
        geom = (np.arange(n) % 4).astype(np.uint8)
        x, t = aug(img, lab, geom, input_type=input_type)
        xp, tp = D.prep_batch(dev(img), dev(lab), dev(geom), input_type)
        assert torch.equal(bits(x), bits(xp)) and torch.equal(bits(t), bits(tp))
        check(img, lab, geom, input_type=input_type)
    x, t = aug(img, lab, None, input_type=input_type)  # geom NULL: no flip
    xp, tp = D.prep_batch(dev(img), dev(lab), None, input_type)
    assert torch.equal(bits(x), bits(xp)) and torch.equal(bits(t), bits(tp))


@pytest.mark.parametrize("input_type", TYPES)
def test_all_eight_orientations(input_type):
    """One orientation per image at 8 x 8; the target follows the image (the labels are a function of the pixel)."""
    _, img, lab = case(8, 8, 8, 12)
    lab = np.where(img[..., 0] >= 128, 255, 0).astype(np.uint8)
    x, t, oi, ol = check(img, lab, np.arange(8), input_type=input_type)
    assert np.array_equal(ol, np.where(oi[..., 0] >= 128, 255, 0))
    if input_type == "RGB":  # channel 0 of x is (r / 255 - 0.5) / 0.5: >= 128 exactly where it is positive
        assert torch.equal(t, (x[:, 0] > 0).float())
    for k in range(8):  # the mirror's orientation is predict --tta's T_k, written out
        src = img[k].transpose(1, 0, 2) if k & 4 else img[k]
        src = src[::-1] if k & 2 else src
        assert np.array_equal(oi[k], src[:, ::-1] if k & 1 else src)


def test_a_transposed_image_must_be_square():
    for h, w in ((8, 16), (7, 8)):
        _, img, lab = case(3, h, w, 13)
        for transposed in (None, True):  # read back from geom, or declared by the caller
            with pytest.raises(K.SelunetError, match="h == w"):
                aug(img, lab, [0, 4, 1], transposed=transposed)
        check(img, lab, [0, 3, 1])  # without bit 2 a non-square batch is right
    torch.cuda.synchronize()


def test_c_abi_argument_checks():
    _, img, lab = case(2, 8, 8, 14)
    di, dl = dev(img), dev(lab)
    x, t = torch.empty(2, 3, 8, 8, device=DEV), torch.empty(2, 8, 8, device=DEV)
    g, k = dev(np.zeros(2, np.uint8)), dev(np.zeros(2, np.uint32))

    def call(img=di, geom=g, glass=None, key=None, lut=None, table=None, tr=0, h=8, w=8, mode=0, x=x, t=t):
        K.call("selunet_prep_batch_aug", K.ptr(img), K.ptr(dl), K.ptr(geom), K.ptr(glass), K.ptr(key), K.ptr(lut),
               K.ptr(table), tr, 2, h, w, mode, K.ptr(x) if torch.is_tensor(x) else x, K.ptr(t), K.stream_ptr())

    call()
    for kw, msg in ((dict(mode=3), "mode"), (dict(mode=-1), "mode"), (dict(h=16, w=4, tr=1), "h == w"),
                    (dict(geom=None, tr=1), "geom"), (dict(w=6), "multiple of 4"), (dict(x=K.ptr(x) + 4), "16-B"),
                    (dict(glass=g), "glass"), (dict(glass=g, key=k), "glass"), (dict(img=None), "bad arguments")):
        with pytest.raises(K.SelunetError, match=msg):
            call(**kw)
    # the Python checks in front of the call
    for bad in (dict(geom=[0]), dict(glass=[0, 1]), dict(glass=[0, 1, 0], keys=[1, 2]),
                dict(lut=np.zeros((2, 3, 128), np.uint8))):
        with pytest.raises(ValueError):
            aug(img, np.zeros((2, 8, 8), np.uint8), **{"geom": [0, 0], **bad})
    with pytest.raises(ValueError):
        aug(img, np.zeros((2, 8, 4), np.uint8), [0, 0])
    with pytest.raises(RuntimeError, match="keys must be a contiguous cuda int32"):
        D.prep_batch_aug(di, dl, g, g, torch.zeros(2, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- glass
@pytest.mark.parametrize("input_type", TYPES)
@pytest.mark.parametrize("side", [8, 12])
def test_glass_quadrants_with_every_orientation(side, input_type):
    """n = 32: every (quadrant, orientation) pair. 8 x 8: the quadrant edge on a 4-pixel group; 12 x 12: inside
    one. Painted bytes are the mirror's, the target there is 0, the rest is the oriented image untouched."""
    n = 32
    rng, img, lab = case(n, side, side, 15)
    lab[:] = 255
    glass, geom = np.arange(n) // 8 + 1, np.arange(n) % 8
    keys = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    x, t, oi, ol = check(img, lab, geom, glass, keys, input_type=input_type)
    plain, _ = AR.augment_bytes(img, lab, geom)
    for b in range(n):
        m = AR.quadrant_mask(side, side, int(glass[b]))  # output coordinates, whatever the orientation
        assert m.sum() == (side // 2) ** 2
        assert np.array_equal(oi[b][m], AR.glass_bytes(side, side, keys[b], TABLE)[m])
        assert np.array_equal(oi[b][~m], plain[b][~m])
        assert (t[b].cpu().numpy()[m] == 0).all() and (t[b].cpu().numpy()[~m] == 1).all()


def test_glass_noise_follows_the_key_alone():
    """Two images with one key are painted alike, whatever the image, its place in the batch or its orientation;
    another key paints differently; non-square and odd sizes slice as the reference (hh = h // 2)."""
    for h, w in ((8, 8), (7, 8), (8, 16)):
        rng, img, lab = case(4, h, w, 16)
        keys = np.array([77, 0xFFFFFFFF, 77, 78], np.uint32)
        x, t, oi, ol = check(img, lab, [0, 1, 3, 2], [4, 4, 4, 4], keys)
        m = AR.quadrant_mask(h, w, 4)
        assert m.sum() == (h - h // 2) * (w - w // 2)
        m = torch.from_numpy(m).to(DEV)
        assert torch.equal(x[0][:, m], x[2][:, m]) and not torch.equal(x[0][:, m], x[3][:, m])
        assert not torch.equal(x[0][:, m], x[1][:, m])
    # glass 0 and a NULL glass are the same call
    a = aug(img, lab, [0, 1, 3, 2], [0, 0, 0, 0], keys)
    b = aug(img, lab, [0, 1, 3, 2])
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


# ----------------------------------------------------------------------------- colour
@pytest.mark.parametrize("input_type", TYPES)
def test_colour_tables(input_type):
    n, side = 4, 12
    rng, img, lab = case(n, side, side, 17)
    lut = luts(rng, n)
    assert len({lut[b].tobytes() for b in range(n)}) == n
    check(img, lab, None, None, None, lut, input_type)
    # glass bypasses the table: painted pixels equal those of the same call without one
    keys = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    glass = [1, 2, 3, 4]
    x, t, oi, _ = check(img, lab, [0, 5, 2, 7], glass, keys, lut, input_type)
    x0, t0 = aug(img, lab, [0, 5, 2, 7], glass, keys, None, input_type)
    for b in range(n):
        m = torch.from_numpy(AR.quadrant_mask(side, side, glass[b])).to(DEV)
        assert torch.equal(bits(x[b][:, m]), bits(x0[b][:, m])) and not torch.equal(bits(x[b][:, ~m]), bits(x0[b][:, ~m]))
    assert torch.equal(t, t0)  # the label never goes through the table
    # the identity table is no table
    ident = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8), (n, 3, 256)))
    xi, ti = aug(img, lab, [0, 5, 2, 7], glass, keys, ident, input_type)
    assert torch.equal(bits(xi), bits(x0)) and torch.equal(ti, t0)


# ----------------------------------------------------------------------------- everything at once
def all_together(n, side, seed):
    rng, img, lab = case(n, side, side, seed)
    geom = (np.array([5, 2, 7, 4, 1, 6, 3, 0])[np.arange(n) % 8]).astype(np.uint8)
    glass = (np.array([3, 1, 4, 0, 2, 4])[np.arange(n) % 6]).astype(np.uint8)
    keys = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    return img, lab, geom, glass, keys, luts(rng, n)


@pytest.mark.parametrize("input_type", TYPES)
def test_all_three_with_different_parameters_per_image(input_type):
    check(*all_together(3, 12, 18), input_type)


GRIDS = (-1, 3, 1)


def under_grids(run):
    """run() -> {name: device tensor} at SELUNET_OPT_IO_GRID = -1, 3 and 1 (the previous value put back); the capped
    runs must equal the default one bit for bit (the helper of tests/test_gpu_io_loops.py, restated)."""
    prev = K.set_option("IO_GRID", -1)
    try:
        res = []
        for g in GRIDS:
            K.set_option("IO_GRID", g)
            assert K.set_option("IO_GRID", g) == g  # the option reads back
            res.append(run())
            torch.cuda.synchronize()
    finally:
        K.set_option("IO_GRID", prev)
    for g, r in zip(GRIDS[1:], res[1:]):
        for k, v in res[0].items():
            assert torch.equal(bits(v), bits(r[k])), f"IO_GRID = {g}: {k} differs from the default grid's"
    return res[0]


@pytest.mark.parametrize("extras", [True, False])
@pytest.mark.parametrize("input_type", TYPES)
def test_loop_wraps_under_a_capped_grid(input_type, extras):
    """6 x 24 x 24: 864 work items, so three workgroups (768 threads) pass twice, the second time ragged, and one
    workgroup four times; outputs NaN-filled first, so an element left unwritten shows. extras False: orientations
    alone, which the launcher gives the kernel variant without the glass and colour code."""
    n, side = 6, 24
    items = n * side * (side // 4)
    assert items > 3 * 256 and items % (3 * 256) and items % 256
    img, lab, geom, glass, keys, lut = all_together(n, side, 19)
    if not extras:
        glass = keys = lut = None
    d = [dev(a) for a in (img, lab, geom, glass, keys, lut)]
    table = dev(TABLE)
    cin = 2 if input_type == "GH" else 3

    def run():
        x = torch.full((n, cin, side, side), float("nan"), device=DEV)
        t = torch.full((n, side, side), float("nan"), device=DEV)
        K.call("selunet_prep_batch_aug", *[K.ptr(a) for a in d], K.ptr(table), 1, n, side, side,
               {"RGB": 0, "GH": 1, "H_RGB": 2}[input_type], K.ptr(x), K.ptr(t), K.stream_ptr())
        return {"x": x, "t": t}

    got = under_grids(run)
    assert not torch.isnan(got["x"]).any() and not torch.isnan(got["t"]).any()
    x, t, _, _ = check(img, lab, geom, glass, keys, lut, input_type)
    assert torch.equal(bits(got["x"]), bits(x)) and torch.equal(bits(got["t"]), bits(t))


# ----------------------------------------------------------------------------- the loader
def test_batch_loader_with_every_option():
    ds = D.synthetic_patchset(40, 32, seed=3)
    ld = D.BatchLoader(ds, 8, shuffle=True, random_flip=True, device=DEV, seed=5, aug_d4=True, aug_glass=0.5,
                       aug_color=0.3)
    ld.set_epoch(2)
    plan = ld._plan()
    first, second = list(ld), list(ld)
    assert len(first) == len(second) == len(plan) == 5
    seen = np.zeros(3, bool)
    for (gb, idx, fl, a), (x, t), (x2, t2) in zip(plan, first, second):
        assert torch.equal(bits(x), bits(x2)) and torch.equal(t, t2)
        assert np.array_equal(a.geom & 3, fl)
        img, lab = np.asarray(ds.images)[idx], np.asarray(ds.labels)[idx]
        xe, te, _, _ = check(img, lab, a.geom, a.glass, a.key, AR.color_lut(a.gamma, a.beta))
        assert torch.equal(bits(x), bits(xe)) and torch.equal(t, te)
        seen |= [(a.geom & 4).any(), (a.glass != 0).any(), (np.abs(a.gamma - 1) > 0.05).any()]
    assert seen.all()
    ld.set_epoch(3)
    assert not torch.equal(bits(next(iter(ld))[0]), bits(first[0][0]))


def test_batch_loader_without_options_is_todays():
    ds = D.synthetic_patchset(40, 32, seed=3)
    ld = D.BatchLoader(ds, 8, shuffle=True, random_flip=True, device=DEV, seed=5)
    calls = []
    K.set_call_hook(lambda name, args, fn: (calls.append(name), fn())[1])
    try:
        got = list(ld)
    finally:
        K.set_call_hook(None)
    assert calls == ["selunet_prep_batch_mode"] * 5
    for (gb, idx, fl), (x, t) in zip(ld._plan(), got):
        xe, te = D.prep_batch(dev(np.asarray(ds.images)[idx]), dev(np.asarray(ds.labels)[idx]), dev(fl))
        assert torch.equal(bits(x), bits(xe)) and torch.equal(t, te)


CHILD = """
import sys
from selectivenet_for_semantic_segmentation_binary_amd import train
train.main(sys.argv[1:])
"""


def test_train_cli_end_to_end(tmp_path):
    argv = ("--data_dir synthetic:40 --patch_size 32 --batch_size 8 --n_epoch 1 --steps_per_epoch 2 --val_steps 1 "
            "--model_arch UNet_B --loss BCElogit --selective 1 --aug_d4 1 --aug_glass 0.25 --aug_color 0.1").split()
    r = subprocess.run([sys.executable, "-c", CHILD, *argv, "--model_dir", str(tmp_path)], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    hist = json.load(open(tmp_path / "1-fold" / "log" / "history.json"))
    assert len(hist) == 1
    assert all(np.isfinite(hist[0][k]) for k in ("train_loss", "valid_loss", "train_acc", "valid_acc"))
    assert sum(map(sum, hist[0]["train_cm"])) > 0
