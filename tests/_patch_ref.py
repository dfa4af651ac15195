"""numpy restatements the per-patch report tests share: the integers of `selunet_seg_metrics_rows` and
`selunet_patch_auc` for one image, from np.sort / np.searchsorted, and the reference fixture."""
import os

import numpy as np

F32 = np.float32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_perf_cases.npz")


def _selected(out, sel, t_sel):
    if sel is None:
        return np.ones(out.shape, bool)
    with np.errstate(invalid="ignore"):
        return sel >= F32(t_sel)  # NaN: not selected


def numpy_counts(out, sel, tgt, t_out, t_sel):
    """[cm00, cm01, cm10, cm11, selected, pixels] of one image (cm[label][pred], labels >= 2 left out)."""
    lab = tgt.astype("uint8").astype(np.int64)
    smask = _selected(out, sel, t_sel)
    with np.errstate(invalid="ignore"):
        pred = (out >= F32(t_out)).astype(np.int64)
    m = smask & (lab < 2)
    cm = np.bincount(lab[m] * 2 + pred[m], minlength=4)
    return [int(v) for v in cm] + [int(smask.sum()), int(out.size)]


def numpy_auc(out, sel, tgt, t_sel):
    """[two_u, n_pos, n_neg, n_nan] of one image: per positive, the negatives below it twice plus the
    negatives equal to it = searchsorted left + right in the sorted negatives."""
    lab = tgt.astype("uint8")
    ok = _selected(out, sel, t_sel) & (lab < 2)
    nan = np.isnan(out)
    pos = out[ok & ~nan & (lab == 1)]
    neg = np.sort(out[ok & ~nan & (lab == 0)])
    two_u = int(np.searchsorted(neg, pos, side="left").sum() + np.searchsorted(neg, pos, side="right").sum())
    return [two_u, int(pos.size), int(neg.size), int((ok & nan).sum())]


def fixture_cases():
    """[(name, label uint8, logit fp32, predict uint8, the reference's five outputs)], and its t_out."""
    z = np.load(FIXTURE)
    names = [str(n) for n in z["names"]]
    return [(n, z[f"label_{n}"], z[f"logit_{n}"], z[f"predict_{n}"], z["perf"][i]) for i, n in enumerate(names)], \
        float(z["t_out"])


def same(a, b):
    """== with NaN matching NaN."""
    return (np.isnan(a) and np.isnan(b)) or a == b


def auc_bound(hw):
    """The reference sums its trapezoids in fp64: at most hw + 1 terms, each at most 1."""
    return (hw + 2) * 2.0 ** -52
