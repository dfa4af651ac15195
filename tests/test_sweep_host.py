"""The risk-coverage sweep's host side, without a GPU: `metrics.sweep_curve` / `cut_off_for_coverage`
on hand-made bins, the order of the logit thresholds a cut-off list maps to, the argument validation
of `selunet_seg_metrics_sweep` (rejected before any launch) and the eval CLI's new flags.
"""
import ctypes
import math
import os

import numpy as np
import pytest

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import build as B
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT
from selectivenet_for_semantic_segmentation_binary_amd.eval import parse_arguments, sweep_cut_offs

# bins[b] = {cm00, cm01, cm10, cm11, pixels}; bin 1 holds 2 pixels of a label >= 2 (pixels only),
# bin 2 is empty, so the rows of cut-offs 1 and 2 coincide
BINS = np.array([[1, 0, 0, 1, 2],
                 [2, 1, 0, 3, 8],
                 [0, 0, 0, 0, 0],
                 [4, 0, 1, 2, 7]], np.int64)
CUTS = [0.1, 0.5, 0.9]


def test_sweep_curve_on_hand_made_bins():
    rows = MT.sweep_curve(BINS, CUTS)
    assert [r["s_cut_off"] for r in rows] == CUTS
    want_cm = [[[6, 1], [1, 5]], [[4, 0], [1, 2]], [[4, 0], [1, 2]]]  # sums of the bins above each cut-off
    want_sel = [15, 7, 7]
    for r, cm, sel in zip(rows, want_cm, want_sel):
        cm = np.array(cm, np.float64)
        assert np.array_equal(np.array(r["confusion_matrix"]), cm)
        assert (r["selected"], r["total"]) == (sel, 17)
        assert r["coverage"] == sel / 17 and r["rejection_ratio"] == (17 - sel) / 17
        assert r["Acc"] == MT.pixel_accuracy(cm) and r["risk"] == 1 - MT.pixel_accuracy(cm)
        assert r["mIoU"] == MT.mean_iou(cm)
        assert r["Prec"] == MT.precision(cm).tolist() and r["Recall"] == MT.recall(cm).tolist()
        p, q = MT.precision(cm), MT.recall(cm)
        assert r["F1_Score"] == (2 * p * q / (p + q)).tolist()
        assert r["IoU_class"] == (np.diag(cm) / (cm.sum(1) + cm.sum(0) - np.diag(cm))).tolist()
    with pytest.raises(ValueError):
        MT.sweep_curve(BINS, CUTS[:2])


def test_sweep_curve_row_with_nothing_selected_is_nan():
    rows = MT.sweep_curve(np.array([[3, 1, 2, 4, 11], [0, 0, 0, 0, 0]]), [1.0])
    r = rows[0]
    assert (r["selected"], r["total"], r["coverage"], r["rejection_ratio"]) == (0, 11, 0.0, 1.0)
    assert np.array_equal(np.array(r["confusion_matrix"]), np.zeros((2, 2)))
    for key in ("Acc", "risk", "mIoU"):
        assert math.isnan(r[key]), key
    for key in ("IoU_class", "Prec", "Recall", "F1_Score"):
        assert all(math.isnan(v) for v in r[key]), key


def test_cut_off_for_coverage():
    curve = [{"s_cut_off": c, "coverage": v} for c, v in ((0.1, 0.9), (0.3, 0.75), (0.5, 0.75), (0.7, 0.5), (0.9, 0.0))]
    assert MT.cut_off_for_coverage(curve, 0.75) == 0.5   # exact hit: the largest cut-off still covering it
    assert MT.cut_off_for_coverage(curve, 0.6) == 0.5    # between two rows
    assert MT.cut_off_for_coverage(curve, 0.5) == 0.7
    assert MT.cut_off_for_coverage(curve, 0.0) == 0.9
    assert MT.cut_off_for_coverage(curve, 0.95) is None  # even the smallest cut-off falls short
    rows = MT.sweep_curve(BINS, CUTS)
    assert MT.cut_off_for_coverage(rows, 0.5) == 0.1 and MT.cut_off_for_coverage(rows, 0.4) == 0.9


def test_thresholds_of_a_cut_off_grid_are_ordered():
    cuts, thr = MT.sweep_thresholds(np.linspace(0, 1, 101))
    assert cuts == np.linspace(0, 1, 101).tolist() and thr.dtype == np.float32 and len(thr) == 101
    assert np.all(thr[1:] >= thr[:-1])
    assert len(set(thr.tolist())) == 101
    # cut-off 0: sigmoid(x) > 0 until fp32 exp(-x) overflows; cut-off 1: never
    assert thr[0] < -80 and np.isinf(thr[-1]) and thr[-1] > 0
    assert [float(t) for t in thr] == [MT.logit_threshold("eval", c) for c in cuts]
    cuts, thr = MT.sweep_thresholds([0.5, 0.2, 0.5, 0.9, 0.2])
    assert cuts == [0.2, 0.5, 0.9] and len(thr) == 3
    MT.sweep_thresholds(np.linspace(0.25, 0.75, 256))
    with pytest.raises(ValueError):
        MT.sweep_thresholds(np.linspace(0.25, 0.75, 257))
    with pytest.raises(ValueError):
        MT.sweep_thresholds([])


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(K.lib_path()):
        B.build()
    return K.load()


def test_sweep_invalid_arguments_fail_with_a_message(lib):
    """Rejected on the host before any launch: no device is touched (the pointers are host memory)."""
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 15) & ~15
    out, sel, tgt, thr, bins = a, a + 1024, a + 2048, a + 3072, a + 3584
    good = [out, sel, tgt, 64, 0.0, thr, 3, bins, None]

    def rejected(**kw):
        args = list(good)
        for name, v in kw.items():
            args[("out", "sel", "target", "p", "t_out", "t_sel", "k", "bins").index(name)] = v
        lib.selunet_last_error.restype = ctypes.c_char_p
        rc = lib.selunet_seg_metrics_sweep(*args)
        msg = lib.selunet_last_error()
        assert rc == 1 and msg and b"seg_metrics_sweep" in msg, (kw, rc, msg)
        return msg

    assert b"k must be" in rejected(k=0)
    assert b"k must be" in rejected(k=K.SWEEP_MAX + 1)
    rejected(k=-1)
    for name in ("out", "sel", "target", "t_sel", "bins"):
        assert b"null" in rejected(**{name: None})
    rejected(p=0)
    rejected(p=-4)
    rejected(p=(1 << 40) + 1)
    for name in ("out", "sel", "target"):
        assert b"aligned" in rejected(**{name: a + 4})
    with pytest.raises(RuntimeError):
        K.call("selunet_seg_metrics_sweep", out, sel, tgt, 64, 0.0, thr, 0, bins, None)


def test_eval_cli_sweep_flags():
    a = parse_arguments([])
    assert (a.s_cut_off_sweep, a.s_cut_off_steps, a.target_coverage) == (None, None, None)
    assert sweep_cut_offs(a) is None
    a = parse_arguments("--s_cut_off_sweep 0.5 0.1 0.9 --target_coverage 0.8".split())
    assert sweep_cut_offs(a) == [0.5, 0.1, 0.9] and a.target_coverage == 0.8
    a = parse_arguments("--s_cut_off_steps 4".split())
    assert sweep_cut_offs(a) == [0.0, 0.25, 0.5, 0.75, 1.0] and a.target_coverage is None
    assert len(sweep_cut_offs(parse_arguments("--s_cut_off_steps 255".split()))) == 256
    for bad in ("--s_cut_off_sweep 0.5 --s_cut_off_steps 4", "--target_coverage 0.8", "--s_cut_off_steps 256",
                "--s_cut_off_steps 0"):
        with pytest.raises(SystemExit):
            parse_arguments(bad.split())
