"""The training augmentation restated in numpy (test infrastructure): the glass table, the counter hash, the
colour table and the rule that decides which three bytes and which label byte of a uint8 batch enter the
per-pixel conversion. Written from the description in DESIGN.md §7l, not from data.py or train_io.hip; the
kernel is held to `augment_bytes` bit for bit."""
from __future__ import annotations

from statistics import NormalDist

import numpy as np

from tests import _tta_ref as TR

U32 = np.uint32


def glass_table():
    """uint8 [4096]: T[j] = floor(255 clip(0.96 + 0.005 Phi^-1((j + 0.5) / 4096), 0, 1) + 0.5), in float64."""
    inv = NormalDist().inv_cdf
    t = [int(np.floor(255 * min(1.0, max(0.0, 0.96 + 0.005 * inv((j + 0.5) / 4096))) + 0.5)) for j in range(4096)]
    return np.array(t, np.uint8)


def mix(v):
    """lowbias32 on a uint32 array (arithmetic modulo 2^32)."""
    v = np.atleast_1d(np.asarray(v, U32)).copy()
    v ^= v >> U32(16)
    v *= U32(0x7FEB352D)
    v ^= v >> U32(15)
    v *= U32(0x846CA68B)
    v ^= v >> U32(16)
    return v


def u(key, counter):
    """uint32: mix(mix(key) + counter * 0x9E3779B9), nothing but the key and the counter."""
    with np.errstate(over="ignore"):
        return mix(mix(U32(key)) + np.asarray(counter, U32) * U32(0x9E3779B9))


def color_lut(gamma, beta):
    """uint8 [n,3,256]: floor(255 min(1, exp(-beta) (v / 255)^gamma) + 0.5) for byte v, entry 0 = 0."""
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    v = np.arange(256) / 255.0
    lut = np.floor(255 * np.minimum(1.0, np.exp(-beta)[..., None] * v ** gamma[..., None]) + 0.5).astype(np.uint8)
    lut[..., 0] = 0
    return lut


def quadrant_mask(h, w, q):
    """bool [h,w]: quadrant q = 1..4 (top-left, top-right, bottom-left, bottom-right; hh = h // 2, hw = w // 2,
    sliced as the reference does: [:hh] / [hh:]); all False for q = 0."""
    m = np.zeros((h, w), bool)
    hh, hw = h // 2, w // 2
    rows = slice(None, hh) if q in (1, 2) else slice(hh, None)
    cols = slice(None, hw) if q in (1, 3) else slice(hw, None)
    if q:
        m[rows, cols] = True
    return m


def glass_bytes(h, w, key, table):
    """uint8 [h,w,3]: the glass paint of a whole h x w output, byte (y, x, c) = T[u(key, (y w + x) 3 + c) >> 20]."""
    counter = np.arange(h * w * 3, dtype=np.uint64).astype(U32)
    return table[u(key, counter) >> U32(20)].reshape(h, w, 3)


def augment_bytes(img, lab, geom=None, glass=None, keys=None, lut=None, table=None):
    """(uint8 [n,h,w,3], uint8 [n,h,w]): the bytes that enter the per-pixel conversion and the label truncation.
    Per image: the source in orientation geom (tests/_tta_ref.T: bit 2 transposes, then bit 1 flips the rows,
    then bit 0 the columns), its bytes through lut[b][c], then quadrant glass[b] of the OUTPUT painted with
    glass_bytes (not through the lut) and its label set to 0."""
    n, h, w, _ = img.shape
    oi, ol = np.empty_like(img), np.empty_like(lab)
    for b in range(n):
        g = 0 if geom is None else int(geom[b])
        if g & 4:
            assert h == w, "a transposed image must be square"
        im, lb = np.array(TR.T(g, img[b])), np.array(TR.T(g, lab[b]))
        if lut is not None:
            im = np.stack([lut[b][c][im[..., c]] for c in range(3)], axis=-1)
        q = 0 if glass is None else int(glass[b])
        if q:
            m = quadrant_mask(h, w, q)
            im[m] = glass_bytes(h, w, keys[b], glass_table() if table is None else table)[m]
            lb[m] = 0
        oi[b], ol[b] = im, lb
    return oi, ol
