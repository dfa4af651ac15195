"""Macenko stain normalisation on the device (MI355X path only; the reference has none): an
H&E image from another lab or scanner is brought to the colour distribution the checkpoint was trained on
before it is predicted.

    python -m selectivenet_for_semantic_segmentation_binary_amd.stain fit --input train_a.png train_dir/ \\
        --out target.json
    python -m selectivenet_for_semantic_segmentation_binary_amd.predict ... --stain_norm macenko \\
        --stain_target target.json

The image's two stain vectors and stain strengths are estimated in optical-density space and the image is
re-rendered with those of a target. Four passes over the pixels run on the device, in integer arithmetic
(`selunet_stain_moments`, `_angle_hist`, `_conc_hist`, `_apply`); the linear algebra between them — a 3 x 3
eigendecomposition, two percentiles of a histogram, a 3 x 2 pseudo-inverse — runs here in float64 on a few
numbers. Every pass adds integers, so a fit and a normalised image are the same bits on every run.

* optical density of a byte v: od_q[v] = round(4096 * -ln(max(v, 1) / 255)) (Q12); a pixel is *stained* iff all
  three are >= round(4096 beta) (beta 0.15): bare glass is out, whatever `--tissue` says;
* pass 1: the count, sums and second moments of the stained pixels' optical densities -> covariance -> `eigh`
  -> e1 (largest eigenvalue, component sum > 0), e2 (second, R component >= 0), B = round(2^14 [e1; e2]);
* pass 2: the histogram over K = 1024 bins of the angle of (B[0] . od, B[1] . od) in (-pi/2, pi/2) -> the bins of
  its 1st and 99th percentile -> v = e1 cos phi + e2 sin phi at the bin centres -> HE (hematoxylin, the one
  with the larger R component, first), P = pinv(HE);
* pass 3: per stain the histogram of P . od over 1024 bins of 1/128 -> maxC = the 99th percentile's bin centre;
* pass 4: out = exp_q[T . od], T = HE_target diag(maxC_target / maxC) P, exp_q[i] = round(255 exp(-i / 1024)).

A percentile p of a histogram with m entries is the smallest bin b with cum[b] >= (p m + 99) // 100.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import dataclass

import numpy as np

K_BINS = 1024   # angle bins (SELUNET_STAIN_ANGLE_BINS)
C_BINS = 1024   # concentration bins of 1/128 (SELUNET_STAIN_CONC_BINS)
BETA = 0.15
MIN_STAINED = 4096
T_LIMIT = 1 << 20  # selunet_stain_apply refuses |T_q| >= 2^20: a factor of 64


# ----------------------------------------------------------------------------- tables
def od_table() -> np.ndarray:
    """int32 [256]: round(4096 * -ln(max(v, 1) / 255)); od_q[255] = 0, od_q[0] = od_q[1] = 22697."""
    v = np.maximum(np.arange(256), 1).astype(np.float64)
    return np.rint(4096.0 * -np.log(v / 255.0)).astype(np.int32)


def exp_table() -> np.ndarray:
    """uint8 [5676]: round(255 exp(-i / 1024)) for i = 0 .. ceil(1024 ln 255)."""
    i = np.arange(math.ceil(1024.0 * math.log(255.0)) + 1, dtype=np.float64)
    return np.rint(255.0 * np.exp(-i / 1024.0)).astype(np.uint8)


def dir_table() -> np.ndarray:
    """int32 [K-1][2]: round(2^14 (cos, sin)) of theta_k = -pi/2 + k pi / K, k = 1 .. K-1."""
    theta = -np.pi / 2 + np.arange(1, K_BINS) * np.pi / K_BINS
    return np.rint(16384.0 * np.stack([np.cos(theta), np.sin(theta)], axis=1)).astype(np.int32)


def beta_q_of(beta: float) -> int:
    beta = float(beta)
    if not (math.isfinite(beta) and 0.0 < beta < 5.5):
        raise ValueError(f"stain: beta must be in (0, 5.5), an optical density (got {beta!r})")
    return int(round(4096.0 * beta))


# ----------------------------------------------------------------------------- the fit and its host steps
class StainFitError(ValueError):
    """Nothing can be fitted to the image(s); str() is the reason."""


@dataclass
class StainFit:
    """A stain fit: HE float64 [3,2], the unit optical-density vectors of hematoxylin and eosin as columns;
    maxC float64 [2], the 99th percentile of each stain's concentration; n_stained, the pixels fitted to;
    skipped, those of them outside the half plane of the angle histogram (x <= 0)."""
    HE: np.ndarray
    maxC: np.ndarray
    n_stained: int = 0
    skipped: int = 0

    def __post_init__(self):
        self.HE = np.asarray(self.HE, np.float64)
        self.maxC = np.asarray(self.maxC, np.float64)
        if self.HE.shape != (3, 2) or self.maxC.shape != (2,):
            raise ValueError(f"StainFit: HE must be [3,2] and maxC [2] (got {self.HE.shape}, {self.maxC.shape})")
        if not (np.isfinite(self.HE).all() and np.isfinite(self.maxC).all() and (self.maxC > 0).all()):
            raise ValueError("StainFit: HE must be finite and maxC finite and positive")
        self.n_stained, self.skipped = int(self.n_stained), int(self.skipped)

    def to_json(self) -> dict:
        return {"HE": self.HE.tolist(), "maxC": self.maxC.tolist(), "n_stained": self.n_stained,
                "skipped": self.skipped}

    @classmethod
    def from_json(cls, doc: dict) -> "StainFit":
        return cls(doc["HE"], doc["maxC"], doc.get("n_stained", 0), doc.get("skipped", 0))


# the commonly published reference of Macenko's method
MACENKO_TARGET = StainFit([[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]], [1.9705, 1.0308])


def basis_of(moments):
    """Pass 1's ten words -> (e1, e2) float64 [3] each. The covariance is formed exactly: n M - s s^T in
    Python integers, then one division by n^2 4096^2 in float64, so an image of one colour has covariance 0."""
    m = [int(v) for v in np.asarray(moments).reshape(10)]
    n, s = m[0], m[1:4]
    if n < 1:
        raise StainFitError("no stained pixel")
    second = {(0, 0): m[4], (0, 1): m[5], (0, 2): m[6], (1, 1): m[7], (1, 2): m[8], (2, 2): m[9]}
    scale = float(n) * float(n) * 4096.0 * 4096.0
    cov = np.array([[float(n * second[min(i, j), max(i, j)] - s[i] * s[j]) / scale for j in range(3)]
                    for i in range(3)], np.float64)
    w, v = np.linalg.eigh(cov)  # ascending
    if not w[1] > 0.0:
        raise StainFitError("the second eigenvalue of the optical-density covariance is not positive")
    e1, e2 = v[:, 2].copy(), v[:, 1].copy()
    if e1.sum() < 0.0:
        e1 = -e1
    if e2[0] < 0.0:
        e2 = -e2
    return e1, e2


def basis_q(e1, e2) -> np.ndarray:
    """B = round(2^14 [e1; e2]), int32 [2][3]."""
    return np.rint(16384.0 * np.stack([e1, e2])).astype(np.int32)


def percentile_bin(hist, p: int) -> int:
    """The smallest bin b with cum[b] >= (p m + 99) // 100, m the histogram's sum."""
    cum = np.cumsum(np.asarray(hist).astype(np.uint64))
    return int(np.searchsorted(cum, np.uint64((p * int(cum[-1]) + 99) // 100)))


def vectors_of(angle_hist, e1, e2) -> np.ndarray:
    """Pass 2's K + 1 words -> HE float64 [3,2]."""
    hist = np.asarray(angle_hist).reshape(K_BINS + 1)[:K_BINS]
    bins = [percentile_bin(hist, p) for p in (1, 99)]
    if any(int(hist[b]) == 0 for b in bins):
        raise StainFitError("a percentile bin of the angle histogram is empty")
    if bins[0] == bins[1]:
        raise StainFitError("the 1st and 99th percentile of the angle histogram share a bin: one stain direction")
    vs = []
    for b in bins:
        phi = -np.pi / 2 + (b + 0.5) * np.pi / K_BINS
        v = e1 * np.cos(phi) + e2 * np.sin(phi)
        vs.append(v / np.linalg.norm(v))
    if vs[0][0] < vs[1][0]:
        vs.reverse()
    return np.stack(vs, axis=1)


def pinv_q(HE):
    """(P float64 [2,3], P_q = round(4096 P) int32 [2][3])."""
    P = np.linalg.pinv(np.asarray(HE, np.float64))
    return P, np.rint(4096.0 * P).astype(np.int32)


def max_conc_of(conc_hist) -> np.ndarray:
    """Pass 3's 2 x CB words -> maxC float64 [2]: the centre of each row's 99th-percentile bin."""
    hist = np.asarray(conc_hist).reshape(2, C_BINS)
    return np.array([(percentile_bin(hist[s], 99) + 0.5) / 128.0 for s in range(2)], np.float64)


def transform(fit: StainFit, target: StainFit) -> np.ndarray:
    """T float64 [3,3] = HE_target diag(maxC_target / maxC) pinv(HE): optical densities of the fitted image ->
    optical densities under the target's stains."""
    return target.HE @ np.diag(target.maxC / fit.maxC) @ np.linalg.pinv(fit.HE)


def transform_q(T) -> np.ndarray:
    """T_q = round(2^14 T), int32 [3][3]; ValueError where an entry reaches 2^20."""
    T = np.asarray(T, np.float64)
    if T.shape != (3, 3) or not np.isfinite(T).all():
        raise ValueError(f"stain: T must be a finite [3,3] matrix (got shape {T.shape})")
    T_q = np.rint(16384.0 * T)
    if (np.abs(T_q) >= T_LIMIT).any():
        raise ValueError(f"stain: an entry of T reaches 64 (max |T| {np.abs(T).max():.3g}): outside the integer "
                         "transform's range")
    return T_q.astype(np.int32)


# ----------------------------------------------------------------------------- the four passes on the device
class _Device:
    """The four passes as library calls on cuda uint8 [H,W,3] tensors. The three statistics calls add into
    device words that several images share; `read` brings them to the host."""

    def __init__(self):
        self.tables = {}

    def _tables(self, device):
        import torch
        key = (device.type, device.index)
        if key not in self.tables:
            self.tables[key] = tuple(torch.from_numpy(t).to(device) for t in (od_table(), exp_table(), dir_table()))
        return self.tables[key]

    def image(self, image_u8):
        import torch
        img = image_u8 if torch.is_tensor(image_u8) else torch.from_numpy(np.ascontiguousarray(image_u8))
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or img.numel() == 0:
            raise ValueError(f"stain: the image must be uint8 [H,W,3] RGB (got {img.dtype} {tuple(img.shape)})")
        if img.device.type != "cuda":
            if not torch.cuda.is_available():
                raise RuntimeError("stain runs on the GPU only (no CPU fallback)")
            img = img.to("cuda")
        return img.contiguous()

    def zeros(self, words, like):
        import torch
        return torch.zeros(words, dtype=torch.int64, device=like.device)  # uint64 bits

    def read(self, acc):
        return acc.cpu().numpy().view(np.uint64)

    def moments(self, img, beta_q, acc):
        import torch
        from . import _lib as K
        with torch.cuda.device(img.device):
            K.call("selunet_stain_moments", K.ptr(img), img.shape[0], img.shape[1], K.ptr(self._tables(img.device)[0]),
                   beta_q, K.ptr(acc), K.stream_ptr())

    def angle_hist(self, img, beta_q, B, acc):
        import torch
        from . import _lib as K
        B = np.ascontiguousarray(B, np.int32)
        od, _, dirs = self._tables(img.device)
        with torch.cuda.device(img.device):
            K.call("selunet_stain_angle_hist", K.ptr(img), img.shape[0], img.shape[1], K.ptr(od), beta_q,
                   B.ctypes.data, K.ptr(dirs), K.ptr(acc), K.stream_ptr())

    def conc_hist(self, img, beta_q, P_q, acc):
        import torch
        from . import _lib as K
        P_q = np.ascontiguousarray(P_q, np.int32)
        with torch.cuda.device(img.device):
            K.call("selunet_stain_conc_hist", K.ptr(img), img.shape[0], img.shape[1],
                   K.ptr(self._tables(img.device)[0]), beta_q, P_q.ctypes.data, K.ptr(acc), K.stream_ptr())

    def apply(self, img, T_q):
        import torch
        from . import _lib as K
        T_q = np.ascontiguousarray(T_q, np.int32)
        od, ex, _ = self._tables(img.device)
        out = torch.empty_like(img)
        with torch.cuda.device(img.device):
            K.call("selunet_stain_apply", K.ptr(img), img.shape[0], img.shape[1], K.ptr(od), T_q.ctypes.data, K.ptr(ex),
                   ex.numel(), K.ptr(out), K.stream_ptr())
        return out


_DEVICE = _Device()


def _fit(images, beta, min_stained, kernels):
    """The fit over one or more images: each pass over all of them into one set of integer words, then the
    host step. Returns (StainFit, the images as the passes take them)."""
    k = kernels or _DEVICE
    beta_q = beta_q_of(beta)
    imgs = [k.image(im) for im in images]
    if not imgs:
        raise ValueError("stain: no image to fit")

    def over_images(words, run):
        acc = k.zeros(words, imgs[0])
        for im in imgs:
            run(im, acc)
        return k.read(acc)

    mom = over_images(10, lambda im, acc: k.moments(im, beta_q, acc))
    n = int(mom[0])
    if n < max(1, int(min_stained)):
        raise StainFitError(f"{n} stained pixels, fewer than {max(1, int(min_stained))}")
    e1, e2 = basis_of(mom)
    B = basis_q(e1, e2)
    ang = over_images(K_BINS + 1, lambda im, acc: k.angle_hist(im, beta_q, B, acc))
    HE = vectors_of(ang, e1, e2)
    _, P_q = pinv_q(HE)
    conc = over_images(2 * C_BINS, lambda im, acc: k.conc_hist(im, beta_q, P_q, acc))
    return StainFit(HE, max_conc_of(conc), n, int(ang[K_BINS])), imgs


def fit(image_u8, beta: float = BETA, *, kernels=None) -> StainFit:
    """The stain vectors and strengths of one uint8 [H,W,3] RGB image (numpy, or a torch tensor on any device):
    passes 1-3. StainFitError where nothing can be fitted. `kernels`: the object whose methods are the four
    passes; the default runs them on the GPU (the tests pass their numpy restatement)."""
    return _fit([image_u8], beta, 1, kernels)[0]


def fit_many(images, beta: float = BETA, *, kernels=None) -> StainFit:
    """One fit to several images, a target from a handful of training images: each pass's integer words are
    summed over the images before its host step, so the images count as one."""
    return _fit(list(images), beta, 1, kernels)[0]


def apply(image_u8, T, *, kernels=None):
    """Pass 4: every pixel of the image through T [3,3] on its optical densities. A new image, of the input's
    kind: a numpy array for a numpy array, a cuda tensor for a tensor."""
    k = kernels or _DEVICE
    out = k.apply(k.image(image_u8), transform_q(T))
    return out.cpu().numpy() if isinstance(image_u8, np.ndarray) and not isinstance(out, np.ndarray) else out


def normalize(image_u8, target: StainFit = MACENKO_TARGET, beta: float = BETA, min_stained: int = MIN_STAINED, *,
              kernels=None):
    """Fit the image and re-render it with the target's stains -> (image, info). info: {"applied", "reason",
    "HE", "maxC", "n_stained", "skipped", "T"} (lists and numbers, as they go into predict.json). Where nothing
    can be fitted — fewer than min_stained stained pixels, a covariance without a second direction, an empty or
    shared percentile bin, a transform beyond the integer range — the input comes back unchanged with applied
    False and the reason; nothing is raised."""
    if not isinstance(target, StainFit):
        raise TypeError(f"stain.normalize: target must be a StainFit (got {type(target).__name__})")
    k = kernels or _DEVICE
    info = {"applied": False, "reason": None, "HE": None, "maxC": None, "n_stained": None, "skipped": None, "T": None}
    as_numpy = isinstance(image_u8, np.ndarray)

    def back(img):
        return img.cpu().numpy() if as_numpy and not isinstance(img, np.ndarray) else img

    try:
        got, (img,) = _fit([image_u8], beta, min_stained, k)
    except StainFitError as e:
        info["reason"] = str(e)
        return (image_u8 if as_numpy else k.image(image_u8)), info
    info.update(got.to_json())
    T = transform(got, target)
    info["T"] = T.tolist()
    try:
        T_q = transform_q(T)
    except ValueError as e:
        info["reason"] = str(e)
        return back(img), info
    info["applied"] = True
    return back(k.apply(img, T_q)), info


# ----------------------------------------------------------------------------- CLI
def load_target(path) -> StainFit:
    with open(path) as fh:
        return StainFit.from_json(json.load(fh))


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser(description="Macenko stain fits on the device")
    sub = parser.add_subparsers(dest="command", required=True)
    f = sub.add_parser("fit", help="one stain target from one or more images (the checkpoint's training images)")
    f.add_argument('--input', type=str, nargs='+', required=True, help='image files or directories of images')
    f.add_argument('--out', type=str, required=True, help='the target, a JSON file for predict --stain_target')
    f.add_argument('--beta', type=float, default=BETA, help='a pixel is stained iff every optical density >= beta')
    args = parser.parse_args(argv)
    if not 0.0 < args.beta < 5.5:
        parser.error('--beta must be in (0, 5.5)')
    return args


def main(argv=None):
    from PIL import Image

    from .predict import list_inputs

    args = parse_arguments(sys.argv[1:] if argv is None else argv)
    files = list_inputs(args.input)
    got = fit_many([np.array(Image.open(p).convert("RGB")) for p in files], args.beta)
    doc = dict(got.to_json(), beta=args.beta, inputs=files)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(f"stain fit over {len(files)} images, {got.n_stained} stained pixels ({got.skipped} skipped): HE "
          f"{np.round(got.HE, 4).tolist()}, maxC {np.round(got.maxC, 4).tolist()} -> {args.out}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
