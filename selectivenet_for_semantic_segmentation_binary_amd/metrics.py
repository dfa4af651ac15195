"""On-device training/eval metrics: the per-batch host code of
train.py:211-238 and eval.py:218-246 plus `Evaluator` (utils/compute_metric.py:4-80), with the
[N,H,W] outputs never leaving HBM.

The reference copies every batch's logits to the host, applies a sigmoid in numpy and
thresholds it: `fn_classifier(fn_sigmoid(x))` = `1/(1+exp(-x)) > 0.5`, in float64 during
training (train.py:150,220-221) and in float32 with `--cut_off` / `--s_cut_off` at eval
(eval.py:171,175,230-231,238-240). Both rules are monotone in the fp32 logit, so each equals
`logit >= t` for one fp32 threshold `t`; `logit_threshold` finds that `t` once on the host by
bisection over the ordered fp32 values, evaluating the reference's own numpy expression (so
masks are bit-exact by construction; e.g. t = 1.5612511e-16 for the training rule and
1.2318974e-07 for the eval rule at cut_off 0.5). The device then only
compares and counts (`selunet_seg_metrics`): the 2x2 confusion matrix over selected pixels and
the selected/total pixel counts, accumulated as uint64 across batches.

`SelectiveSweep` does the same for a sorted list of selection cut-offs in one pass
(`selunet_seg_metrics_sweep`): the risk-coverage curve, and `cut_off_for_coverage` to calibrate the
cut-off to a wanted coverage.

`PatchReport` keeps one row per patch in the same pass (`selunet_seg_metrics_rows`,
`selunet_patch_auc`): the counts per image and the exact integer Mann-Whitney statistic of the
prediction logit, from which `patch_performance` forms the reference's unused `get_performance`
(utils/compute_metric.py:93-148) — accuracy, recall, precision, f1 score and ROC AUC per patch.

`BoundaryReport` adds the distance view: an exact on-device Euclidean distance transform
of the label and prediction masks (`selunet_edt_sq`), the `SegMetrics` counts by band of distance to the
label contour (`band_table`: where the network errs and abstains) and per patch the directed Hausdorff
distances and boundary-tolerant scores (`boundary_patch`).

`CalibrationReport` asks whether the scores can be read as probabilities: per view one
`selunet_calibration_bins` call per batch counts the reliability bins of sigmoid(score / T) against an event with
the fixed-point sums behind the Brier score and the NLL, and a fine histogram of the raw score; on the host,
`calibration_edges` places the bins' logit thresholds by the reference's fp32 rule, `calibration_table` /
`calibration_summary` form the table, ECE, top-label ECE, MCE, Brier score and NLL, and `fit_temperature` finds
the temperature that minimises `nll_from_fine`.
"""
from __future__ import annotations

import functools
import warnings

import numpy as np
import torch

from . import _lib as K
from . import parallel


def _ordered(i: int) -> np.float32:
    """fp32 value with rank i in the total order of finite floats (i in [-2^31+2^23.., ...])."""
    if i >= 0:
        return np.array([i], np.int32).view(np.float32)[0]
    return -np.array([-i], np.int32).view(np.float32)[0]


def _rank(f: np.float32) -> int:
    b = int(np.array([f], np.float32).view(np.int32)[0])
    return b if b >= 0 else -(b & 0x7FFFFFFF)


@functools.lru_cache(maxsize=None)
def logit_threshold(rule: str = "train", cut_off: float = 0.5, output_scale: str = "sigmoid") -> float:
    """Smallest fp32 logit x with reference-pred(x) == 1.

    rule 'train': train.py:150,217-221 — fn_sigmoid in float64, then `> 0.5` (fn_classifier,
                  train.py:154); cut_off is fixed at 0.5 there.
    rule 'eval':  eval.py:171,175,229-231 — fn_sigmoid on the float32 array, `> cut_off`.
    output_scale != 'sigmoid': the raw logit is compared (`> cut_off`).
    """
    if rule == "argmax":
        # CE UNet with 2 classes (train.py:207-209, 216-219: np.argmax over the class / selection
        # axis, ties -> class 0): callers pass the fp32 difference x1 - x0, which is > 0 exactly
        # when x1 > x0; the smallest positive fp32 makes `>= t` the strict comparison.
        return float(np.nextafter(np.float32(0), np.float32(1)))
    if output_scale != "sigmoid":
        pred = lambda x: bool(np.array([x], np.float32) > cut_off)  # noqa: E731
    elif rule == "train":
        pred = lambda x: bool((1 / (1 + np.exp(-np.array([x], np.float32).astype("float64")))) > 0.5)  # noqa: E731
    elif rule == "eval":
        pred = lambda x: bool((1 / (1 + np.exp(-np.array([x], np.float32)))) > cut_off)  # noqa: E731
    else:
        raise ValueError(f"unknown threshold rule {rule!r}")
    with np.errstate(over="ignore"):
        return _bisect(pred)


def _bisect(pred) -> float:
    lo, hi = _rank(np.float32(-np.finfo(np.float32).max)), _rank(np.float32(np.finfo(np.float32).max))
    if pred(_ordered(lo)):
        return float(-np.inf)
    if not pred(_ordered(hi)):
        return float(np.inf)
    while hi - lo > 1:  # invariant: pred(lo) false, pred(hi) true
        mid = (lo + hi) // 2
        if pred(_ordered(mid)):
            hi = mid
        else:
            lo = mid
    return float(_ordered(hi))


def _check_planes(who, selective, output, target, selection, per_patch=False, ids=None, noun=None):
    """The argument rules the `add_batch` methods share; `who` names the class in the message."""
    for name, t in (("output", output), ("target", target), ("selection", selection)):
        if t is not None and (t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError(f"{who}.add_batch: {name} must be a contiguous cuda fp32 tensor")
    if per_patch:
        if output.dim() != 3:
            raise ValueError(f"{who}.add_batch: output must be (N, H, W), got {tuple(output.shape)}")
        if target.shape != output.shape or (selection is not None and selection.shape != output.shape):
            raise ValueError(f"{who}.add_batch: output, target and selection must have the same shape")
    elif output.numel() != target.numel() or (selection is not None and selection.numel() != output.numel()):
        raise ValueError(f"{who}.add_batch: output, target and selection must have the same size")
    if selective and selection is None:
        raise ValueError(f"selective {noun or who} needs the selection logits")
    if ids is not None and len(ids) != output.shape[0]:
        raise ValueError(f"{who}.add_batch: {len(ids)} ids for {output.shape[0]} patches")


def _host_sums(counts: torch.Tensor) -> np.ndarray:
    """A device tensor of counts summed over the data-parallel ranks, on the host as int64 (one synchronisation)."""
    c = counts.clone()
    parallel.allreduce_sums(c)
    return c.cpu().numpy().astype(np.int64)


class SegMetrics:
    """Device-side Evaluator (utils/compute_metric.py:4-80) for num_class = 2.

    add_batch(output, target, selection=None) counts one batch without a host copy;
    confusion_matrix() syncs once (and all-reduces across data-parallel ranks).
    """

    def __init__(self, device, selective: bool, rule: str = "train", cut_off: float = 0.5,
                 s_cut_off: float = 0.5, output_scale: str = "sigmoid"):
        self.selective = selective
        self.t_out = logit_threshold(rule, cut_off, output_scale)
        self.t_sel = logit_threshold(rule, s_cut_off, output_scale)
        self.counts = torch.zeros(6, dtype=torch.int64, device=device)  # uint64 bits

    def reset(self):
        self.counts.zero_()

    def add_batch(self, output: torch.Tensor, target: torch.Tensor, selection: torch.Tensor | None = None):
        _check_planes("SegMetrics", self.selective, output, target, selection, noun="Evaluator")
        sel = selection if self.selective else None
        K.call("selunet_seg_metrics", K.ptr(output), K.ptr(sel), K.ptr(target), output.numel(), self.t_out,
               self.t_sel, K.ptr(self.counts), K.stream_ptr())

    def raw(self) -> np.ndarray:
        return _host_sums(self.counts)

    def confusion_matrix(self) -> np.ndarray:
        return self.raw()[:4].reshape(2, 2).astype(np.float64)

    def selected_total(self) -> tuple[int, int]:
        r = self.raw()
        return int(r[4]), int(r[5])


# Evaluator formulas (utils/compute_metric.py:34-80) on a host confusion matrix
def pixel_accuracy(cm):
    return np.diag(cm).sum() / cm.sum()


def mean_iou(cm):
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = np.diag(cm) / (np.sum(cm, axis=1) + np.sum(cm, axis=0) - np.diag(cm))
    return np.nanmean(iou)


def precision(cm):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.diag(cm) / cm.sum(axis=0)


def recall(cm):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.diag(cm) / cm.sum(axis=1)


def dice(cm):
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2 * np.diag(cm) / (np.sum(cm, axis=1) + np.sum(cm, axis=0))


def sweep_thresholds(s_cut_offs, rule: str = "eval", output_scale: str = "sigmoid"):
    """(cut-offs sorted and de-duplicated, their fp32 selection-logit thresholds). The reference's
    rule is monotone in the cut-off, so the thresholds come out non-decreasing (checked): each pixel
    then lies in exactly one bin between two of them. Pure host code."""
    cuts = sorted({float(c) for c in s_cut_offs})
    if not cuts:
        raise ValueError("risk-coverage sweep: no cut-offs")
    if any(np.isnan(c) for c in cuts):
        raise ValueError("risk-coverage sweep: NaN cut-off")
    if len(cuts) > K.SWEEP_MAX:
        raise ValueError(f"risk-coverage sweep: {len(cuts)} distinct cut-offs, at most {K.SWEEP_MAX}")
    thr = np.array([logit_threshold(rule, c, output_scale) for c in cuts], np.float32)
    if np.any(thr[1:] < thr[:-1]):
        raise ValueError(f"risk-coverage sweep: the logit thresholds of {cuts} are not non-decreasing: {thr}")
    return cuts, thr


class SelectiveSweep:
    """Risk-coverage sweep of the selection cut-off in one pass over the data: per batch, one
    `selunet_seg_metrics_sweep` call bins every pixel by how many of the sorted selection thresholds
    its selection logit reaches and counts a 2x2 confusion matrix per bin. `sweep_curve` suffix-sums
    the bins on the host into the counts `SegMetrics` would give at each cut-off alone (integer work:
    bit-exact). The prediction rule (`cut_off`) is fixed, as in `SegMetrics`."""

    def __init__(self, device, s_cut_offs, rule: str = "eval", cut_off: float = 0.5,
                 output_scale: str = "sigmoid"):
        self.s_cut_offs, thr = sweep_thresholds(s_cut_offs, rule, output_scale)
        self.t_out = logit_threshold(rule, cut_off, output_scale)
        self.thresholds = torch.tensor(thr, dtype=torch.float32, device=device)
        self.bins = torch.zeros(len(self.s_cut_offs) + 1, 5, dtype=torch.int64, device=device)  # uint64 bits

    def reset(self):
        self.bins.zero_()

    def add_batch(self, output: torch.Tensor, target: torch.Tensor, selection: torch.Tensor):
        if selection is None:
            raise ValueError("SelectiveSweep.add_batch needs the selection logits")
        _check_planes("SelectiveSweep", True, output, target, selection)
        K.call("selunet_seg_metrics_sweep", K.ptr(output), K.ptr(selection), K.ptr(target), output.numel(),
               self.t_out, K.ptr(self.thresholds), len(self.s_cut_offs), K.ptr(self.bins), K.stream_ptr())

    def raw(self) -> np.ndarray:
        return _host_sums(self.bins)

    def curve(self) -> list:
        return sweep_curve(self.raw(), self.s_cut_offs)


def sweep_curve(bins, s_cut_offs) -> list:
    """One row per cut-off (ascending) from the [(k+1), 5] bin counts of `SelectiveSweep.raw()`: a pixel
    of bin b is selected at cut-off j exactly when b > j, so row j is the sum of the bins above j."""
    bins = np.asarray(bins, np.int64)
    cuts = [float(c) for c in s_cut_offs]
    if bins.shape != (len(cuts) + 1, 5):
        raise ValueError(f"sweep_curve: bins of shape {bins.shape} for {len(cuts)} cut-offs")
    suffix = np.cumsum(bins[::-1], axis=0)[::-1]
    total = int(bins[:, 4].sum())
    rows = []
    for j, c in enumerate(cuts):
        cm = suffix[j + 1, :4].reshape(2, 2).astype(np.float64)
        selected = int(suffix[j + 1, 4])
        prec, rec = precision(cm), recall(cm)
        with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # nanmean of an all-NaN row: nothing selected
            acc = float(pixel_accuracy(cm))
            f1 = 2 * (prec * rec) / (prec + rec)
            iou_class = np.diag(cm) / (cm.sum(1) + cm.sum(0) - np.diag(cm))
            miou = float(mean_iou(cm))
        rows.append({"s_cut_off": c, "confusion_matrix": cm.tolist(), "selected": selected, "total": total,
                     "coverage": selected / total if total else float("nan"),
                     "rejection_ratio": (total - selected) / max(total, 1),
                     "Acc": acc, "risk": 1.0 - acc, "mIoU": miou, "IoU_class": iou_class.tolist(),
                     "Prec": prec.tolist(), "Recall": rec.tolist(), "F1_Score": f1.tolist()})
    return rows


def cut_off_for_coverage(curve, target):
    """The largest cut-off of the curve whose coverage is >= target (coverage does not increase with
    the cut-off); None when even the smallest cut-off selects less."""
    ok = [r["s_cut_off"] for r in curve if r["coverage"] >= target]
    return max(ok) if ok else None


# ----------------------------------------------------------------------------- per-patch report
PATCH_METRICS = ("accuracy", "recall", "precision", "f1_score", "auc_score")
PATCH_COUNTS = ("cm00", "cm01", "cm10", "cm11", "n_pos", "n_neg", "two_u", "n_nan")


def patch_performance(cm, two_u, n_pos, n_neg) -> dict:
    """The reference's `get_performance` (utils/compute_metric.py:93-148) from one patch's integers:
    cm[label][pred] the 2x2 confusion matrix, two_u / n_pos / n_neg of `selunet_patch_auc`. Its rules
    as written, in Python numbers like its own `len()` ratios: accuracy = (TP+TN)/(C1+C0) (NaN where
    the reference would divide by zero), recall NaN without a label-1 pixel, precision NaN without a
    predicted-1 pixel; f1 = 2rp/(r+p) whenever r + p != 0 — its `recall != np.NaN` guard is always
    true, so a NaN recall or precision propagates and r + p == 0 leaves NaN; AUC = two_u /
    (2 n_pos n_neg), ties at one half as `roc_auc_score`, NaN when a class is missing (its try/except)."""
    (tn, fp), (fn, tp) = ((int(v) for v in row) for row in cm)
    c1, c0, p1 = fn + tp, tn + fp, fp + tp
    nan = float("nan")
    accuracy = (tp + tn) / (c1 + c0) if c1 + c0 else nan
    recall = tp / c1 if c1 else nan
    precision = tp / p1 if p1 else nan
    f1 = nan
    if recall + precision != 0:
        f1 = 2 * recall * precision / (recall + precision)
    n_pos, n_neg = int(n_pos), int(n_neg)
    auc = int(two_u) / (2 * n_pos * n_neg) if n_pos and n_neg else nan
    return {"accuracy": accuracy, "recall": recall, "precision": precision, "f1_score": f1, "auc_score": auc}


def patch_row(counts, auc, prefix="") -> dict:
    """The report fields of one patch from its six `selunet_seg_metrics_rows` counts and its four
    `selunet_patch_auc` words."""
    cm = [[int(counts[0]), int(counts[1])], [int(counts[2]), int(counts[3])]]
    two_u, n_pos, n_neg, n_nan = (int(v) for v in auc)
    row = {"cm00": cm[0][0], "cm01": cm[0][1], "cm10": cm[1][0], "cm11": cm[1][1], "n_pos": n_pos, "n_neg": n_neg,
           "two_u": two_u, "n_nan": n_nan}
    row.update(patch_performance(cm, two_u, n_pos, n_neg))
    return {prefix + k: v for k, v in row.items()}


class _PatchRows:
    """The row store of a per-patch report: per batch one device tensor [passes][sections] of uint64 bits, a
    section being [n][width] words of the batch's n patches, and the patches' ids. Nothing is copied until
    `patches()`, which copies everything once."""

    def __init__(self):
        self._batches = []  # (n, device int64 tensor)
        self._ids = []

    def add(self, n, buf, ids):
        self._batches.append((n, buf))
        self._ids.extend([None] * n if ids is None else [str(i) for i in ids])

    def patches(self, widths):
        """(index, id, words) per patch in the order fed: words[pass][section] is the patch's row of that section
        (sections of `widths` words per patch); the id defaults to patch_{index}."""
        if not self._batches:
            return
        host = torch.cat([b.reshape(-1) for _, b in self._batches]).cpu().numpy()
        at = index = 0
        for n, buf in self._batches:
            part = host[at:at + buf.numel()].reshape(buf.shape[0], -1)
            at += buf.numel()
            sections = [[s.reshape(n, -1) for s in np.split(p, np.cumsum(widths)[:-1] * n)] for p in part]
            for i in range(n):
                pid = self._ids[index] if self._ids[index] is not None else f"patch_{index}"
                yield index, pid, [[s[i] for s in p] for p in sections]
                index += 1


def _finite_stats(values) -> tuple:
    """(count, mean, median) of the finite values; the mean and the median are NaN when there is none."""
    v = np.array(values, np.float64)
    finite = v[np.isfinite(v)]
    if not len(finite):
        return 0, float("nan"), float("nan")
    return len(finite), float(finite.mean()), float(np.median(finite))


class PatchReport:
    """One row per patch in the pass eval already makes: per batch, `selunet_seg_metrics_rows` (the
    Evaluator's counts per image) and `selunet_patch_auc` (the exact integer Mann-Whitney statistic of
    the prediction logit) over all pixels and, with `selective`, again over the selected ones. The
    per-batch row tensors stay on the device (no host synchronisation per batch); `rows()` copies once."""

    def __init__(self, device, selective: bool, rule: str = "eval", cut_off: float = 0.5,
                 s_cut_off: float = 0.5, output_scale: str = "sigmoid"):
        self.device = device
        self.selective = bool(selective)
        self.t_out = logit_threshold(rule, cut_off, output_scale)
        self.t_sel = logit_threshold(rule, s_cut_off, output_scale)
        self.reset()

    def reset(self):
        self._rows = _PatchRows()  # per batch [passes][n*6 + n*4]

    def add_batch(self, output: torch.Tensor, target: torch.Tensor, selection: torch.Tensor | None = None, ids=None):
        _check_planes("PatchReport", self.selective, output, target, selection, per_patch=True, ids=ids)
        n, hw = output.shape[0], output.shape[1] * output.shape[2]
        passes = [None, selection] if self.selective else [None]
        buf = torch.zeros(len(passes), n * 10, dtype=torch.int64, device=output.device)
        stream = K.stream_ptr()
        for k, sel in enumerate(passes):
            K.call("selunet_seg_metrics_rows", K.ptr(output), K.ptr(sel), K.ptr(target), n, hw, self.t_out,
                   self.t_sel, buf[k].data_ptr(), stream)
            K.call("selunet_patch_auc", K.ptr(output), K.ptr(sel), K.ptr(target), n, hw, self.t_sel,
                   buf[k].data_ptr() + n * 6 * 8, stream)
        self._rows.add(n, buf, ids)

    def rows(self) -> list:
        rows = []
        for index, pid, words in self._rows.patches((6, 4)):
            counts, auc = words[0]
            row = {"index": index, "id": pid, "pixels": int(counts[5])}
            row.update(patch_row(counts, auc))
            if self.selective:
                counts, auc = words[1]
                row["selected"] = int(counts[4])
                row["coverage"] = row["selected"] / row["pixels"]
                row.update(patch_row(counts, auc, prefix="sel_"))
            rows.append(row)
        return rows


def patch_report_columns(rows) -> tuple:
    """Column order of patch_performance.csv for these rows (with or without the selection fields)."""
    cols = ("index", "id", "pixels") + PATCH_COUNTS + PATCH_METRICS
    if rows and "selected" in rows[0]:
        cols += ("selected", "coverage") + tuple("sel_" + c for c in PATCH_COUNTS + PATCH_METRICS)
    return cols


def patch_report_summary(rows) -> dict:
    """Number of patches, of patches with a NaN AUC, and the mean and median of the finite AUCs (NaN
    when there is none); with selection the same over the selected pixels' AUCs."""
    doc = {"patches": len(rows)}
    for prefix in ("", "sel_") if rows and "selected" in rows[0] else ("",):
        finite, mean, median = _finite_stats([r[prefix + "auc_score"] for r in rows])
        doc.update({prefix + "nan_auc": len(rows) - finite, prefix + "mean_auc": mean, prefix + "median_auc": median})
    return doc


# ----------------------------------------------------------------------------- boundary distances
BAND_COUNTS = ("cm00", "cm01", "cm10", "cm11", "selected", "pixels")
BAND_COLUMNS = ("band", "r_lo", "r_hi") + BAND_COUNTS + (
    "pixel_share", "coverage", "errors", "risk", "rejected", "rejected_share", "error_share",
    "cum_pixel_share", "cum_rejected_share", "cum_error_share")
BOUNDARY_WORDS = ("fp_max_d2", "fn_max_d2", "fp_within", "fn_within", "fp", "fn")
BOUNDARY_METRICS = ("hausdorff", "hd_pred_to_label", "hd_label_to_pred", "tolerant_accuracy", "tolerant_tumor_iou")


def band_edges_sq(radii) -> np.ndarray:
    """floor(r^2) of the band radii, in float64: a pixel lies within r of the contour exactly when its
    integer squared distance is <= floor(r^2). The radii and their floored squares must be strictly
    increasing from >= 1 (two radii between the same two integers' roots would make an empty band), at
    most `BAND_MAX` of them, below the largest distance of a 4096 x 4096 plane."""
    r = np.asarray(radii, np.float64).reshape(-1)
    if r.size < 1 or r.size > K.BAND_MAX:
        raise ValueError(f"boundary bands: {r.size} radii, between 1 and {K.BAND_MAX} are allowed")
    if not np.all(np.isfinite(r)) or np.any(r < 1) or np.any(np.diff(r) <= 0):
        raise ValueError(f"boundary bands: the radii must be finite, >= 1 and strictly increasing, got {r.tolist()}")
    r2 = np.floor(r * r)
    if np.any(np.diff(r2) <= 0) or r2[-1] >= K.EDT_NONE:
        raise ValueError(f"boundary bands: the floored squares {r2.tolist()} of the radii must be strictly "
                         f"increasing and below 2^31 - 1")
    return r2


def boundary_distance_sq(x: torch.Tensor, t: float, out: torch.Tensor | None = None) -> torch.Tensor:
    """`selunet_edt_sq` of an (N, H, W) contiguous cuda fp32 tensor: int32 (N, H, W), the squared Euclidean
    distance of every pixel to the nearest pixel of the other class of its image (foreground: x >= t),
    `K.EDT_NONE` throughout an image of one class. `out` (same shape, int32, contiguous) is overwritten."""
    if x.device.type != "cuda" or x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError("boundary_distance_sq: x must be a contiguous cuda fp32 tensor")
    if x.dim() != 3:
        raise ValueError(f"boundary_distance_sq: x must be (N, H, W), got {tuple(x.shape)}")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    elif out.device != x.device or out.dtype != torch.int32 or not out.is_contiguous():
        raise RuntimeError("boundary_distance_sq: out must be a contiguous int32 tensor on x's device")
    elif out.shape != x.shape:
        raise ValueError(f"boundary_distance_sq: out of shape {tuple(out.shape)} for x of {tuple(x.shape)}")
    n, h, w = x.shape
    K.call("selunet_edt_sq", K.ptr(x), float(t), n, h, w, K.ptr(out), K.stream_ptr())
    return out


def _ratio(a, b):
    return a / b if b else float("nan")


def band_table(bins, radii) -> list:
    """One row per band from the [(k+2), 6] counts of `BoundaryReport.raw_bands()`: bands 0..k by distance
    to the label contour (r_lo < d <= r_hi, r_hi = inf for band k), then band k+1, the patches without a
    contour (r_lo = r_hi = NaN). errors = cm01 + cm10 (over the selected pixels), risk = errors / selected,
    coverage = selected / pixels, rejected = pixels - selected; the shares are of the totals over all bands
    (NaN where the total is 0) and the cum_ columns their running sums in band order."""
    bins = np.asarray(bins, np.int64)
    radii = [float(r) for r in radii]
    k = len(radii)
    if bins.shape != (k + 2, 6):
        raise ValueError(f"band_table: bins of shape {bins.shape} for {k} radii")
    pixels, selected = bins[:, 5], bins[:, 4]
    errors, rejected = bins[:, 1] + bins[:, 2], pixels - selected
    tot_p, tot_r, tot_e = int(pixels.sum()), int(rejected.sum()), int(errors.sum())
    lo = [0.0] + radii + [float("nan")]
    hi = radii + [float("inf"), float("nan")]
    rows, cum = [], [0, 0, 0]
    for b in range(k + 2):
        cum = [cum[0] + int(pixels[b]), cum[1] + int(rejected[b]), cum[2] + int(errors[b])]
        row = {"band": b, "r_lo": lo[b], "r_hi": hi[b]}
        row.update({name: int(bins[b, i]) for i, name in enumerate(BAND_COUNTS)})
        row.update({"pixel_share": _ratio(int(pixels[b]), tot_p), "coverage": _ratio(int(selected[b]), int(pixels[b])),
                    "errors": int(errors[b]), "risk": _ratio(int(errors[b]), int(selected[b])),
                    "rejected": int(rejected[b]), "rejected_share": _ratio(int(rejected[b]), tot_r),
                    "error_share": _ratio(int(errors[b]), tot_e), "cum_pixel_share": _ratio(cum[0], tot_p),
                    "cum_rejected_share": _ratio(cum[1], tot_r), "cum_error_share": _ratio(cum[2], tot_e)})
        rows.append(row)
    return rows


def _root(d2) -> float:
    d2 = int(d2)
    return float("inf") if d2 >= K.EDT_NONE else float(np.sqrt(np.float64(d2)))


def boundary_patch(words, counts, prefix="") -> dict:
    """The boundary fields of one patch from its six `selunet_boundary_rows` words and its six
    `selunet_seg_metrics_rows` counts. hd_pred_to_label = sqrt(word 0), the directed Hausdorff distance from
    the predicted region to the label region (0 without a false positive, inf when there is one and the
    label mask is empty); hd_label_to_pred = sqrt(word 1) the converse; hausdorff their maximum. The tolerant
    scores count an error within the tolerance of the other mask as a hit of the tumor class:
    tolerant_accuracy = (TP + TN + near) / counted, tolerant_tumor_iou = (TP + near) / (TP + FP + FN), NaN
    where the denominator is 0."""
    w = [int(v) for v in words]
    tn, fp, fn, tp = (int(v) for v in counts[:4])
    if (fp, fn) != (w[4], w[5]):
        raise ValueError(f"boundary_patch: {w[4]} / {w[5]} false positives / negatives against a confusion "
                         f"matrix with {fp} / {fn}")
    near = w[2] + w[3]
    row = dict(zip(BOUNDARY_WORDS, w))
    a, b = _root(w[0]), _root(w[1])
    row.update({"hausdorff": max(a, b), "hd_pred_to_label": a, "hd_label_to_pred": b,
                "tolerant_accuracy": _ratio(tp + tn + near, tn + fp + fn + tp),
                "tolerant_tumor_iou": _ratio(tp + near, tp + fp + fn)})
    return {prefix + k: v for k, v in row.items()}


class BoundaryReport:
    """Where the network errs and abstains, by distance to the annotation's contour, in the pass eval
    already makes. Per batch: the exact distance transform (`selunet_edt_sq`) of the target at 0.5 and of
    the output at its logit threshold into two int32 planes kept between batches, `selunet_boundary_bands`
    (the six `SegMetrics` counts per distance band, over the selected pixels when `selective`), and per patch
    `selunet_boundary_rows` + `selunet_seg_metrics_rows` over all pixels and, when `selective`, again over
    the selected ones. Nothing synchronises per batch: `bands()` / `rows()` copy once."""

    def __init__(self, device, selective: bool, radii=(1, 2, 4, 8, 16), tolerance: float = 2.0,
                 rule: str = "eval", cut_off: float = 0.5, s_cut_off: float = 0.5, output_scale: str = "sigmoid"):
        self.device = device
        self.selective = bool(selective)
        self.radii = [float(r) for r in radii]
        self.r2 = band_edges_sq(self.radii).astype(np.int32)
        self._r2c = (K.c_int32 * len(self.r2))(*[int(v) for v in self.r2])
        self.tolerance = float(tolerance)
        if not np.isfinite(self.tolerance) or self.tolerance < 0 or self.tolerance ** 2 >= K.EDT_NONE:
            raise ValueError(f"BoundaryReport: tolerance must be finite, >= 0 and below 2^15.5, got {tolerance}")
        self.tol_sq = int(np.floor(np.float64(self.tolerance) ** 2))
        self.t_out = logit_threshold(rule, cut_off, output_scale)
        self.t_sel = logit_threshold(rule, s_cut_off, output_scale)
        self.bins = torch.zeros(len(self.r2) + 2, 6, dtype=torch.int64, device=device)  # uint64 bits
        self._store = None  # int32, 2 planes [n][h][w]: the distances of the target and of the prediction
        self.reset()

    def reset(self):
        self.bins.zero_()
        self._rows = _PatchRows()  # per batch [passes][n*6 + n*6]

    def add_batch(self, output: torch.Tensor, target: torch.Tensor, selection: torch.Tensor | None = None, ids=None):
        _check_planes("BoundaryReport", self.selective, output, target, selection, per_patch=True, ids=ids)
        n, hw = output.shape[0], output.shape[1] * output.shape[2]
        if hw % 4 or hw > 1 << 20 or max(output.shape[1:]) > K.EDT_MAX_SIDE:  # before anything is counted
            raise ValueError(f"BoundaryReport.add_batch: patches of {tuple(output.shape[1:])}: H * W must be a "
                             f"multiple of 4 and at most 2^20, H and W at most {K.EDT_MAX_SIDE}")
        if self._store is None or self._store.numel() < 2 * output.numel() or self._store.device != output.device:
            self._store = torch.empty(2 * output.numel(), dtype=torch.int32, device=output.device)
        planes = self._store[:2 * output.numel()].view(2, *output.shape)
        d2_target = boundary_distance_sq(target, 0.5, out=planes[0])
        d2_pred = boundary_distance_sq(output, self.t_out, out=planes[1])
        stream = K.stream_ptr()
        sel = selection if self.selective else None
        K.call("selunet_boundary_bands", K.ptr(output), K.ptr(sel), K.ptr(target), K.ptr(d2_target), n, hw,
               self.t_out, self.t_sel, self._r2c, len(self.r2), K.ptr(self.bins), stream)
        passes = [None, selection] if self.selective else [None]
        buf = torch.zeros(len(passes), n * 12, dtype=torch.int64, device=output.device)
        for k, s in enumerate(passes):
            K.call("selunet_boundary_rows", K.ptr(output), K.ptr(s), K.ptr(target), K.ptr(d2_target), K.ptr(d2_pred),
                   n, hw, self.t_out, self.t_sel, self.tol_sq, buf[k].data_ptr(), stream)
            K.call("selunet_seg_metrics_rows", K.ptr(output), K.ptr(s), K.ptr(target), n, hw, self.t_out,
                   self.t_sel, buf[k].data_ptr() + n * 6 * 8, stream)
        self._rows.add(n, buf, ids)

    def raw_bands(self) -> np.ndarray:
        return _host_sums(self.bins)

    def bands(self) -> list:
        return band_table(self.raw_bands(), self.radii)

    def rows(self) -> list:
        rows = []
        for index, pid, words in self._rows.patches((6, 6)):
            row = {"index": index, "id": pid, "pixels": int(words[0][1][5])}
            row.update(boundary_patch(*words[0]))
            if self.selective:
                row["selected"] = int(words[1][1][4])
                row.update(boundary_patch(*words[1], prefix="sel_"))
            rows.append(row)
        return rows


def boundary_report_columns(rows) -> tuple:
    """Column order of patch_boundary.csv for these rows (with or without the selection fields)."""
    cols = ("index", "id", "pixels") + BOUNDARY_WORDS + BOUNDARY_METRICS
    if rows and "selected" in rows[0]:
        cols += ("selected",) + tuple("sel_" + c for c in BOUNDARY_WORDS + BOUNDARY_METRICS)
    return cols


def boundary_report_summary(rows) -> dict:
    """Number of patches, of patches with an infinite and with a zero Hausdorff distance, and the mean and
    median of the finite ones (NaN when there is none); with selection the same over the selected pixels."""
    doc = {"patches": len(rows)}
    for prefix in ("", "sel_") if rows and "selected" in rows[0] else ("",):
        hd = [r[prefix + "hausdorff"] for r in rows]
        finite, mean, median = _finite_stats(hd)
        doc.update({prefix + "infinite_hausdorff": len(hd) - finite, prefix + "zero_hausdorff": hd.count(0),
                    prefix + "mean_hausdorff": mean, prefix + "median_hausdorff": median})
    return doc


# ----------------------------------------------------------------------------- calibration
CALIBRATION_BIN_COLUMNS = ("bin", "lo", "hi", "non_events", "events", "sum_score", "sum_brier", "sum_nll", "n",
                           "event_rate", "mean_score", "gap")
CALIBRATION_VIEWS = ("tumor", "tumor_selected", "selection")
_FRAC = float(1 << K.CALIB_FRAC_BITS)
_NLL = float(1 << K.CALIB_NLL_BITS)


def calibration_edges(k, temperature: float = 1.0):
    """(the k - 1 interior edges j / k of k equal-width probability bins, their fp32 logit thresholds): the
    smallest fp32 score x whose probability reaches past the edge by the reference's fp32 rule,
    `1/(1+exp(-(x/T))) > j/k`. At temperature 1 these are `sweep_thresholds(..., rule="eval")`, so the middle
    edge is `logit_threshold("eval", 0.5)` and the bins line up with the Evaluator's prediction. k is even
    (the top-label fold pairs bin k/2 + j with bin k/2 - 1 - j) and in [2, 256]. Pure host code."""
    if isinstance(k, bool) or int(k) != k or not 2 <= int(k) <= K.CALIB_MAX_EDGES + 1 or int(k) % 2:
        raise ValueError(f"calibration: the number of bins must be even and in [2, {K.CALIB_MAX_EDGES + 1}], got {k}")
    k, t = int(k), float(temperature)
    if not np.isfinite(t) or not t > 0:
        raise ValueError(f"calibration: the temperature must be finite and > 0, got {temperature}")
    cuts = [j / k for j in range(1, k)]
    if t == 1.0:
        return sweep_thresholds(cuts, rule="eval")
    t32 = np.float32(t)
    with np.errstate(over="ignore"):
        thr = np.array([_bisect(lambda x, c=c: bool((1 / (1 + np.exp(-(np.array([x], np.float32) / t32)))) > c))
                        for c in cuts], np.float32)
    if np.any(thr[1:] < thr[:-1]):
        raise ValueError(f"calibration: the logit thresholds at temperature {t} are not non-decreasing: {thr}")
    return cuts, thr


def _calibration_rows(rows):
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != 5 or rows.shape[0] < 2 or rows.shape[0] % 2:
        raise ValueError(f"calibration: rows of shape {rows.shape}, expected [k][5] with k even")
    return [[int(v) for v in r] for r in rows]  # Python integers: sums of 2^33 pixels x 2^30 pass 2^63


def calibration_table(rows, k) -> list:
    """One row per reliability bin from the [k][5] words {non-events, events, sum P, sum B, sum L} of
    `selunet_calibration_bins`: the bin's probability range lo = b/k, hi = (b+1)/k, n = events + non-events,
    event_rate = events / n, mean_score = sum P / 2^30 / n, gap = event_rate - mean_score (NaN for an empty bin)."""
    rows = _calibration_rows(rows)
    if len(rows) != k:
        raise ValueError(f"calibration_table: {len(rows)} rows for {k} bins")
    table = []
    for b, (n0, n1, sp, sb, sl) in enumerate(rows):
        n = n0 + n1
        rate, mean = _ratio(n1, n), _ratio(sp / _FRAC, n)
        table.append({"bin": b, "lo": b / k, "hi": (b + 1) / k, "non_events": n0, "events": n1, "sum_score": sp,
                      "sum_brier": sb, "sum_nll": sl, "n": n, "event_rate": rate, "mean_score": mean,
                      "gap": rate - mean})
    return table


def calibration_summary(rows) -> dict:
    """pixels N; ECE = sum n_b / N |event_rate - mean_score| and MCE, the largest such gap of a non-empty bin;
    Brier = sum B / 2^30 / N; NLL = sum L / 2^20 / N (nats, a pixel capped at 1024); and the top-label view,
    the fold of bin k/2 + j with bin k/2 - 1 - j into confidence bin j (confidence in [1/2 + j/k, 1/2 + (j+1)/k]):
    its confidence sum is P above the middle and n 2^30 - P below, its hits are the events above and the
    non-events below; top_label_accuracy their share of N. NaN throughout without a pixel."""
    rows = _calibration_rows(rows)
    k = len(rows)
    total = sum(r[0] + r[1] for r in rows)
    ece, mce = 0.0, 0.0
    for n0, n1, sp, _, _ in rows:
        if n0 + n1:
            gap = abs(n1 / (n0 + n1) - sp / _FRAC / (n0 + n1))
            ece += (n0 + n1) / total * gap
            mce = max(mce, gap)
    top, top_ece, hits = [], 0.0, 0
    for j in range(k // 2):
        (u0, u1, up, _, _), (l0, l1, lp, _, _) = rows[k // 2 + j], rows[k // 2 - 1 - j]
        n, correct = u0 + u1 + l0 + l1, u1 + l0
        conf = up + ((l0 + l1) << K.CALIB_FRAC_BITS) - lp
        acc, mean = _ratio(correct, n), _ratio(conf / _FRAC, n)
        top.append({"bin": j, "lo": 0.5 + j / k, "hi": 0.5 + (j + 1) / k, "n": n, "correct": correct,
                    "sum_confidence": conf, "accuracy": acc, "mean_confidence": mean, "gap": acc - mean})
        if n:
            top_ece += n / total * abs(acc - mean)
        hits += correct
    nan = float("nan")
    return {"pixels": total, "ece": ece if total else nan, "mce": mce if total else nan,
            "brier": _ratio(sum(r[3] for r in rows) / _FRAC, total), "nll": _ratio(sum(r[4] for r in rows) / _NLL, total),
            "top_label_ece": top_ece if total else nan, "top_label_accuracy": _ratio(hits, total), "top_label": top}


def fine_midpoints() -> np.ndarray:
    """The score that stands for each cell of the fine histogram: the midpoint (c - 2049 + 0.5) / 64 of cells
    1..4096, and -32 / +32 for the two open end cells."""
    x = (np.arange(K.CALIB_FINE_CELLS, dtype=np.float64) - 2049 + 0.5) / 64
    x[0], x[-1] = -32.0, 32.0
    return x


def _fine(fine):
    fine = np.asarray(fine)
    if fine.shape != (K.CALIB_FINE_CELLS, 2):
        raise ValueError(f"calibration: fine histogram of shape {fine.shape}, expected ({K.CALIB_FINE_CELLS}, 2)")
    return fine.astype(np.float64)


def _softplus(v):
    return np.maximum(v, 0) + np.log1p(np.exp(-np.abs(v)))


def nll_from_fine(fine, temperature: float = 1.0) -> float:
    """Mean NLL (nats per pixel) of sigmoid(score / temperature) read off the fine histogram [4098][2]
    (`fine[cell][event]`), every pixel standing at its cell's `fine_midpoints`. A midpoint is at most 1/128
    from its score and softplus is 1-Lipschitz, so this is within 1 / (128 T) of the exact mean while no
    |score| >= 32. NaN without a pixel."""
    f = _fine(fine)
    x = fine_midpoints() / float(temperature)
    n = f.sum()
    return float((f[:, 0] * _softplus(x) + f[:, 1] * _softplus(-x)).sum() / n) if n else float("nan")


def fit_temperature(fine) -> dict:
    """The temperature T = 1/a that minimises `nll_from_fine`, a in [1/64, 64]. The NLL is convex in a, so the
    root of its derivative sum x (n sigmoid(a x) - n_1) is found by Newton steps kept inside a bracket
    (bisected on log a where a step leaves it), run to a relative step below 1e-9; the end of the range where
    the NLL is monotone over it. Returns the temperature, the NLL at T = 1 and at the fitted T (all NaN
    without a pixel)."""
    f = _fine(fine)
    n = f.sum(1)
    if not n.sum():
        return {"temperature": float("nan"), "nll": float("nan"), "nll_fitted": float("nan")}
    x = fine_midpoints()

    def slope(a):
        s = 0.5 * (1 + np.tanh(0.5 * a * x))  # sigmoid without overflow
        return float((x * (n * s - f[:, 1])).sum()), float((x * x * n * s * (1 - s)).sum())

    lo, hi = 1 / 64, 64.0
    if slope(lo)[0] >= 0:
        a = lo
    elif slope(hi)[0] <= 0:
        a = hi
    else:
        a = 1.0
        for _ in range(200):
            g, h = slope(a)
            if g > 0:
                hi = a
            elif g < 0:
                lo = a
            else:
                break
            nxt = a - g / h if h > 0 else 0.0
            if not lo < nxt < hi:
                nxt = float(np.sqrt(lo * hi))
            step, a = abs(nxt - a), nxt
            if step <= 1e-9 * a:
                break
    return {"temperature": 1 / a, "nll": nll_from_fine(fine, 1.0), "nll_fitted": nll_from_fine(fine, 1 / a)}


class CalibrationReport:
    """Whether the scores can be read as probabilities, in the pass eval already makes: per batch
    one `selunet_calibration_bins` call per view,
      tumor:          sigmoid(output / temperature) against the label, over all pixels;
      tumor_selected: the same over the selected pixels (with `select_eval`);
      selection:      sigmoid(selection) against "the prediction is right", over all pixels, at temperature 1
                      (with a selective network): does the selection score track correctness.
    Nothing synchronises per batch; `raw()` copies once (and all-reduces across data-parallel ranks), `report()`
    adds each view's `calibration_table`, `calibration_summary` and `fit_temperature`."""

    def __init__(self, device, selective: bool, select_eval: bool, bins: int = 20, temperature: float = 1.0,
                 cut_off: float = 0.5, s_cut_off: float = 0.5):
        self.selective, self.select_eval = bool(selective), bool(select_eval)
        if self.select_eval and not self.selective:
            raise ValueError("CalibrationReport: select_eval needs a selective network")
        self.k, self.temperature = int(bins), float(temperature)
        self.views = ["tumor"] + (["tumor_selected"] if self.select_eval else []) + (
            ["selection"] if self.selective else [])
        _, tumor = calibration_edges(bins, temperature)
        self._edges = {"tumor": torch.tensor(tumor, dtype=torch.float32, device=device)}
        if self.selective:
            self._edges["selection"] = torch.tensor(calibration_edges(bins)[1], dtype=torch.float32, device=device)
        self.t_out = logit_threshold("eval", cut_off)
        self.t_sel = logit_threshold("eval", s_cut_off)
        # per view, uint64 bits: bins [k][5], fine [4098][2], misc [2]
        self._words = self.k * 5 + K.CALIB_FINE_CELLS * 2 + 2
        self.counts = torch.zeros(len(self.views), self._words, dtype=torch.int64, device=device)

    def reset(self):
        self.counts.zero_()

    def view_temperature(self, view: str) -> float:
        return 1.0 if view == "selection" else self.temperature

    def add_batch(self, output: torch.Tensor, target: torch.Tensor, selection: torch.Tensor | None = None):
        _check_planes("CalibrationReport", self.selective, output, target, selection)
        stream = K.stream_ptr()
        for i, view in enumerate(self.views):
            if view == "selection":
                score, out, sel, event, edges = selection, output, None, 1, self._edges["selection"]
            else:
                score, out, event, edges = output, None, 0, self._edges["tumor"]
                sel = selection if view == "tumor_selected" else None
            base = self.counts[i].data_ptr()
            K.call("selunet_calibration_bins", K.ptr(score), K.ptr(out), K.ptr(sel), K.ptr(target), output.numel(),
                   event, self.t_out, self.t_sel, K.ptr(edges), self.k - 1, 1.0 / self.view_temperature(view), base,
                   base + self.k * 5 * 8, base + (self._words - 2) * 8, stream)

    def raw(self) -> dict:
        host = _host_sums(self.counts)
        at = self.k * 5
        return {view: {"bins": host[i, :at].reshape(self.k, 5), "fine": host[i, at:-2].reshape(-1, 2),
                       "misc": host[i, -2:]} for i, view in enumerate(self.views)}

    def report(self) -> dict:
        doc = {"bins": self.k, "views": {}}
        for view, r in self.raw().items():
            edges = self._edges["selection" if view == "selection" else "tumor"].cpu().numpy()
            doc["views"][view] = {"temperature": self.view_temperature(view),
                                  "edge_logits": [float(v) for v in edges],
                                  "nan_scores": int(r["misc"][0]), "other_labels": int(r["misc"][1]),
                                  "summary": calibration_summary(r["bins"]), "fit": fit_temperature(r["fine"]),
                                  "table": calibration_table(r["bins"], self.k)}
        return doc
