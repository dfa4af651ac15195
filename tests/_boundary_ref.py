"""numpy oracle of the boundary-distance metrics, independent of the package: the exact
squared distance to the other class by brute force (all pairs) and in the separable form, the band and
per-image counts, and the host formulas restated."""
import math

import numpy as np

NONE = 2 ** 31 - 1
F32 = np.float32


def foreground(x, t):
    with np.errstate(invalid="ignore"):
        return np.asarray(x, F32) >= F32(t)  # a NaN compares false: background


def brute_d2(mask):
    """[h][w] bool -> int64 [h][w]: the smallest squared distance to a pixel of the other class, over all
    pairs of pixels; NONE when the image holds one class."""
    h, w = mask.shape
    m = mask.ravel()
    if m.all() or not m.any():
        return np.full((h, w), NONE, np.int64)
    ys, xs = np.divmod(np.arange(h * w, dtype=np.int32), w)
    out = np.empty(h * w, np.int64)
    for a in range(0, h * w, 512):  # 512 query pixels at a time: 512 x hw words
        b = min(a + 512, h * w)
        d = (ys[a:b, None] - ys[None, :]) ** 2 + (xs[a:b, None] - xs[None, :]) ** 2
        out[a:b] = np.where(m[a:b, None] != m[None, :], d, NONE).min(1)
    return out.reshape(h, w)


def brute_d2_batch(x, t):
    return np.stack([brute_d2(foreground(img, t)) for img in x])


def separable_d2(mask):
    """The same in the separable form (column distances, then a minimum over each row), O(h w^2)."""
    h, w = mask.shape
    far = 1 << 28
    g = np.empty((2, h, w), np.int64)  # g[c]: squared vertical distance to the nearest pixel of class c
    rows = np.arange(h)[:, None]
    for c in (0, 1):
        is_c = mask == bool(c)
        above = np.maximum.accumulate(np.where(is_c, rows, -far), axis=0)
        below = np.minimum.accumulate(np.where(is_c, rows, far)[::-1], axis=0)[::-1]
        g[c] = np.minimum(np.minimum(rows - above, below - rows), far) ** 2
    dx2 = (np.arange(w)[:, None] - np.arange(w)[None, :]) ** 2
    out = np.empty((h, w), np.int64)
    for y in range(h):
        other = np.where(mask[y][:, None], g[0, y][None, :], g[1, y][None, :])  # [x][x']: g of the other class
        out[y] = (dx2 + other).min(1)
    return np.where(out >= far, NONE, out)


def states(out, sel, tgt, t_out, t_sel):
    """(selected, label, pred) of flat arrays under selunet_seg_metrics' rules."""
    with np.errstate(invalid="ignore"):
        selected = np.ones(out.shape, bool) if sel is None else sel >= F32(t_sel)
        pred = out >= F32(t_out)
    lab = tgt.astype(np.uint8).astype(np.int64)
    return selected, lab, pred


def six_counts(selected, lab, pred, where):
    cells = [int((where & selected & (lab == a) & (pred == bool(b))).sum()) for a in (0, 1) for b in (0, 1)]
    return cells + [int((where & selected).sum()), int(where.sum())]


def numpy_bands(out, sel, tgt, d2, r2, t_out, t_sel):
    """[k+2][6] of flat arrays: the six counts over the pixels of each band of d2."""
    selected, lab, pred = states(out, sel, tgt, t_out, t_sel)
    r2 = [int(v) for v in r2]
    k = len(r2)
    lo = [0] + r2
    bands = [(d2 > lo[j]) & (d2 <= r2[j]) if j else d2 <= r2[0] for j in range(k)]
    bands.append((d2 > r2[-1]) & (d2 != NONE))
    bands.append(d2 == NONE)
    assert sum(int(b.sum()) for b in bands) == d2.size
    return np.array([six_counts(selected, lab, pred, b) for b in bands], np.int64)


def numpy_rows(out, sel, tgt, d2t, d2p, t_out, t_sel, tol_sq):
    """[n][6] of [n][hw] arrays: max d2_target over the false positives, max d2_pred over the false
    negatives, their numbers within tol_sq, their numbers."""
    selected, lab, pred = states(out, sel, tgt, t_out, t_sel)
    fp, fn = selected & (lab == 0) & pred, selected & (lab == 1) & ~pred
    return np.stack([np.where(fp, d2t, 0).max(1), np.where(fn, d2p, 0).max(1), (fp & (d2t <= tol_sq)).sum(1),
                     (fn & (d2p <= tol_sq)).sum(1), fp.sum(1), fn.sum(1)], 1).astype(np.int64)


def div(a, b):
    return a / b if b else float("nan")


def band_formulas(bins, radii):
    """Per band: pixels and their share, coverage, risk = errors / selected, the band's share of all
    rejected pixels and of all selected errors, and the running sums of the three shares."""
    bins = [[int(v) for v in row] for row in bins]
    k = len(radii)
    tot_pix = sum(r[5] for r in bins)
    tot_rej = sum(r[5] - r[4] for r in bins)
    tot_err = sum(r[1] + r[2] for r in bins)
    rows, c_pix, c_rej, c_err = [], 0, 0, 0
    for b, r in enumerate(bins):
        err, rej = r[1] + r[2], r[5] - r[4]
        c_pix, c_rej, c_err = c_pix + r[5], c_rej + rej, c_err + err
        rows.append({"band": b,
                     "r_lo": float("nan") if b == k + 1 else 0.0 if b == 0 else float(radii[b - 1]),
                     "r_hi": float("nan") if b == k + 1 else float("inf") if b == k else float(radii[b]),
                     "cm00": r[0], "cm01": r[1], "cm10": r[2], "cm11": r[3], "selected": r[4], "pixels": r[5],
                     "pixel_share": div(r[5], tot_pix), "coverage": div(r[4], r[5]), "errors": err,
                     "risk": div(err, r[4]), "rejected": rej, "rejected_share": div(rej, tot_rej),
                     "error_share": div(err, tot_err), "cum_pixel_share": div(c_pix, tot_pix),
                     "cum_rejected_share": div(c_rej, tot_rej), "cum_error_share": div(c_err, tot_err)})
    return rows


def patch_formulas(words, cm):
    """hausdorff and its two directed parts, the tolerant accuracy and tumor IoU of one patch from its six
    words and its confusion matrix [tn, fp, fn, tp]."""
    w = [int(v) for v in words]
    tn, fp, fn, tp = (int(v) for v in cm)
    a = math.inf if w[0] == NONE else math.sqrt(w[0])
    b = math.inf if w[1] == NONE else math.sqrt(w[1])
    near = w[2] + w[3]
    return {"fp_max_d2": w[0], "fn_max_d2": w[1], "fp_within": w[2], "fn_within": w[3], "fp": w[4], "fn": w[5],
            "hausdorff": max(a, b), "hd_pred_to_label": a, "hd_label_to_pred": b,
            "tolerant_accuracy": div(tp + tn + near, tn + fp + fn + tp),
            "tolerant_tumor_iou": div(tp + near, tp + fp + fn)}


def same(a, b):
    """Equal, NaN equal to NaN."""
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b
