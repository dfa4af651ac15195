"""Macenko stain normalisation restated in numpy (test infrastructure): the four device passes in
int64, the host steps between them, the whole integer pipeline, a float64 textbook Macenko (arctan2,
np.percentile, log and exp) and a synthetic H&E generator. Written from the definition in DESIGN.md §7m, not
from stain.py or csrc/stain.hip; nothing here comes from the reference project, which has no stain
normalisation."""
from __future__ import annotations

import math

import numpy as np

K, CB = 1024, 1024
BETA, MIN_STAINED = 0.15, 4096
TARGET_HE = np.array([[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]])
TARGET_MAXC = np.array([1.9705, 1.0308])
# Re-fitting a normalised 96 x 128 synthetic image (seeds 0, 1, 2, normalize_int then fit_int, measured on the CPU)
# gives vectors 0.012 / 0.018 / 0.011 deg (hematoxylin) and 1.238 / 0.891 / 1.044 deg (eosin) from the target's:
# the bound of the re-fit tests is the worst of them plus 0.5 deg.
REFIT_DEG = 1.238 + 0.5


# ----------------------------------------------------------------------------- tables
def od_table():
    return np.array([round(4096 * -math.log(max(v, 1) / 255)) for v in range(256)], np.int32)


def exp_table():
    return np.array([round(255 * math.exp(-i / 1024)) for i in range(math.ceil(1024 * math.log(255)) + 1)], np.uint8)


def dir_table():
    return np.array([(round(16384 * math.cos(-math.pi / 2 + k * math.pi / K)),
                      round(16384 * math.sin(-math.pi / 2 + k * math.pi / K))) for k in range(1, K)], np.int32)


OD_Q, EXP_Q, DIRS = od_table(), exp_table(), dir_table()


def beta_q_of(beta=BETA):
    return int(round(4096 * beta))


# ----------------------------------------------------------------------------- the four passes, int64
def od_of(image):
    """int64 [H*W,3]: the Q12 optical densities of every pixel."""
    return OD_Q[np.asarray(image).reshape(-1, 3)].astype(np.int64)


def stained_od(image, beta_q):
    od = od_of(image)
    return od[(od >= beta_q).all(axis=1)]


def moments(image, beta_q):
    """uint64 [10]: {n, sum r, g, b, sum rr, rg, rb, gg, gb, bb} over the stained pixels."""
    od = stained_od(image, beta_q)
    r, g, b = od[:, 0], od[:, 1], od[:, 2]
    vals = [len(od), r.sum(), g.sum(), b.sum(), (r * r).sum(), (r * g).sum(), (r * b).sum(), (g * g).sum(),
            (g * b).sum(), (b * b).sum()]
    return np.array([int(v) for v in vals], np.uint64)


def angle_hist(image, beta_q, B, check_monotone=True):
    """uint64 [K+1]: per stained pixel with x > 0 the bin #{k in 1..K-1: cq_k y - sq_k x >= 0}, counted over all
    k (no search); x <= 0 goes to word K. With check_monotone the predicate is asserted true up to the bin and
    false above it for every pixel: what a search by halving relies on."""
    od = stained_od(image, beta_q)
    B = np.asarray(B, np.int64)
    x, y = od @ B[0], od @ B[1]
    out = np.zeros(K + 1, np.uint64)
    out[K] = int((x <= 0).sum())
    x, y = x[x > 0], y[x > 0]
    cq, sq = DIRS[:, 0].astype(np.int64), DIRS[:, 1].astype(np.int64)
    for a in range(0, len(x), 8192):
        pred = cq[None, :] * y[a:a + 8192, None] - sq[None, :] * x[a:a + 8192, None] >= 0  # [n, K-1]
        bins = pred.sum(axis=1)
        if check_monotone:
            assert (pred == (np.arange(1, K)[None, :] <= bins[:, None])).all()
        out[:K] += np.bincount(bins, minlength=K).astype(np.uint64)
    return out


def conc_hist(image, beta_q, P_q):
    """uint64 [2][CB]: per stained pixel and stain the bin clamp((P_q[s] . od) >> 17, 0, CB - 1)."""
    od = stained_od(image, beta_q)
    c = od @ np.asarray(P_q, np.int64).T  # [n,2], Q24
    bins = np.clip(c >> 17, 0, CB - 1)
    return np.stack([np.bincount(bins[:, s], minlength=CB) for s in range(2)]).astype(np.uint64)


def apply_int(image, T_q, exp_q=EXP_Q):
    """uint8 image: out_c = exp_q[clamp((T_q[c] . od + 2^15) >> 16, 0, n_exp - 1)] for every pixel."""
    o = od_of(image) @ np.asarray(T_q, np.int64).T
    idx = np.clip((o + (1 << 15)) >> 16, 0, len(exp_q) - 1)
    return np.asarray(exp_q)[idx].reshape(np.asarray(image).shape).astype(np.uint8)


# ----------------------------------------------------------------------------- the host steps
def pct_bin(hist, p):
    """The smallest bin b with cum[b] >= (p m + 99) // 100."""
    cum = [0]
    for v in hist:
        cum.append(cum[-1] + int(v))
    want = (p * cum[-1] + 99) // 100
    return next(b for b in range(len(hist)) if cum[b + 1] >= want)


def basis_of(mom):
    """(e1, e2, second eigenvalue): covariance (n M - s s^T) / (n^2 4096^2) with the numerator in exact integers."""
    m = [int(v) for v in mom]
    n, s = m[0], m[1:4]
    M = [[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]]
    scale = float(n) * float(n) * 4096.0 * 4096.0
    cov = np.array([[float(n * M[i][j] - s[i] * s[j]) / scale for j in range(3)] for i in range(3)])
    w, v = np.linalg.eigh(cov)
    e1, e2 = v[:, 2].copy(), v[:, 1].copy()
    return (e1 if e1.sum() >= 0 else -e1), (e2 if e2[0] >= 0 else -e2), w[1]


def he_of(e1, e2, phis):
    vs = [e1 * np.cos(p) + e2 * np.sin(p) for p in phis]
    vs = [v / np.linalg.norm(v) for v in vs]
    return np.stack(vs if vs[0][0] >= vs[1][0] else vs[::-1], axis=1)


def transform_of(HE, maxC, target_HE=TARGET_HE, target_maxC=TARGET_MAXC):
    return target_HE @ np.diag(target_maxC / maxC) @ np.linalg.pinv(HE)


def fit_int(images, beta=BETA, min_stained=1):
    """The integer fit over a list of images (their integer words summed per pass). Returns a dict with HE, maxC,
    n_stained, skipped and the intermediate integers, or {"reason": ...} where nothing can be fitted."""
    bq = beta_q_of(beta)
    mom = sum(moments(im, bq).astype(object) for im in images)
    n = int(mom[0])
    if n < max(1, min_stained):
        return {"reason": "too few stained pixels", "n_stained": n}
    e1, e2, w1 = basis_of(mom)
    if not w1 > 0:
        return {"reason": "second eigenvalue", "n_stained": n}
    B = np.rint(16384.0 * np.stack([e1, e2])).astype(np.int32)
    ang = sum(angle_hist(im, bq, B).astype(object) for im in images)
    bins = [pct_bin(ang[:K], p) for p in (1, 99)]
    if any(int(ang[b]) == 0 for b in bins):
        return {"reason": "empty percentile bin", "n_stained": n}
    if bins[0] == bins[1]:
        return {"reason": "one direction", "n_stained": n}
    HE = he_of(e1, e2, [-np.pi / 2 + (b + 0.5) * np.pi / K for b in bins])
    P_q = np.rint(4096.0 * np.linalg.pinv(HE)).astype(np.int32)
    conc = sum(conc_hist(im, bq, P_q).astype(object) for im in images)
    maxC = np.array([(pct_bin(conc[s], 99) + 0.5) / 128.0 for s in range(2)])
    return {"HE": HE, "maxC": maxC, "n_stained": n, "skipped": int(ang[K]), "moments": mom, "B": B, "angle_hist": ang,
            "P_q": P_q, "conc_hist": conc, "bins": bins}


def normalize_int(image, target_HE=TARGET_HE, target_maxC=TARGET_MAXC, beta=BETA, min_stained=MIN_STAINED):
    """(image, fit dict with "applied" and, when applied, "T" and "T_q"): the whole integer pipeline."""
    f = fit_int([image], beta, min_stained)
    f["applied"] = False
    if "HE" not in f:
        return image, f
    f["T"] = transform_of(f["HE"], f["maxC"], target_HE, target_maxC)
    T_q = np.rint(16384.0 * f["T"])
    if (np.abs(T_q) >= 1 << 20).any():
        f["reason"] = "transform out of range"
        return image, f
    f["T_q"], f["applied"] = T_q.astype(np.int32), True
    return apply_int(image, f["T_q"]), f


class Kernels:
    """The four passes behind the interface stain.py drives the device through (its `kernels=` argument)."""

    def image(self, image_u8):
        img = np.ascontiguousarray(image_u8)
        assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
        return img

    def zeros(self, words, like):
        return np.zeros(words, np.uint64)

    def read(self, acc):
        return acc

    def moments(self, img, beta_q, acc):
        acc += moments(img, beta_q)

    def angle_hist(self, img, beta_q, B, acc):
        acc += angle_hist(img, beta_q, B)

    def conc_hist(self, img, beta_q, P_q, acc):
        acc += conc_hist(img, beta_q, P_q).reshape(-1)

    def apply(self, img, T_q):
        return apply_int(img, T_q)


# ----------------------------------------------------------------------------- float64 textbook Macenko
def od_float(image):
    return -np.log(np.maximum(np.asarray(image).reshape(-1, 3).astype(np.float64), 1.0) / 255.0)


def fit_float(image, beta=BETA, alpha=1.0, shift=(0.0, 0.0)):
    """Macenko et al. 2009 in float64: eigh of the covariance of the stained pixels' optical densities,
    arctan2 angles in the plane of the two leading eigenvectors, their alpha and 100 - alpha percentiles, the two
    unit vectors (larger R first), least-squares concentrations and their 99th percentile. Textbook code takes
    the last percentile over all pixels; here it is over the stained ones, the population of the integer fit.
    The stained rule and the sign conventions are the integer fit's. shift: added to the two angles (radians),
    for the fit's own sensitivity to one angular bin."""
    od = od_float(image)
    od = od[(od >= beta).all(axis=1)]
    w, v = np.linalg.eigh(np.cov(od.T))
    e1, e2 = v[:, 2], v[:, 1]
    e1, e2 = (e1 if e1.sum() >= 0 else -e1), (e2 if e2[0] >= 0 else -e2)
    phi = np.arctan2(od @ e2, od @ e1)
    HE = he_of(e1, e2, [np.percentile(phi, alpha) + shift[0], np.percentile(phi, 100 - alpha) + shift[1]])
    conc = np.linalg.lstsq(HE, od.T, rcond=None)[0]
    return {"HE": HE, "maxC": np.percentile(conc, 99, axis=1), "n_stained": len(od)}


def apply_float(image, T):
    """round(255 exp(-T od)) per pixel, clipped to a byte."""
    o = od_float(image) @ np.asarray(T, np.float64).T
    return np.clip(np.rint(255.0 * np.exp(-o)), 0, 255).astype(np.uint8).reshape(np.asarray(image).shape)


def normalize_float(image, target_HE=TARGET_HE, target_maxC=TARGET_MAXC, beta=BETA):
    f = fit_float(image, beta)
    return apply_float(image, transform_of(f["HE"], f["maxC"], target_HE, target_maxC)), f


def angle_deg(a, b):
    """The angle between two vectors, in degrees."""
    c = float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


# ----------------------------------------------------------------------------- synthetic H&E
STAIN_H = np.array([0.65, 0.70, 0.29])  # Ruifrok & Johnston's hematoxylin and eosin, as unit vectors below
STAIN_E = np.array([0.07, 0.99, 0.11])


def synthetic_he(H=96, W=128, seed=0, glass=0.2, he=(STAIN_H, STAIN_E), shape=(2.0, 2.0), scale=(0.3, 0.16)):
    """An H x W x 3 uint8 image of two known unit stain vectors: gamma-distributed concentrations per pixel,
    about `glass` of the pixels with none, rendered as 255 exp(-(cH h + cE e)) plus Gaussian noise of one grey
    level, rounded and clipped."""
    rng = np.random.Generator(np.random.PCG64(seed))
    h, e = (np.asarray(v, np.float64) / np.linalg.norm(v) for v in he)
    c = rng.gamma(shape, scale, (H, W, 2))
    c[rng.random((H, W)) < glass] = 0.0
    od = c[..., :1] * h + c[..., 1:] * e
    img = 255.0 * np.exp(-od) + rng.standard_normal((H, W, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
