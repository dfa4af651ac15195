"""The host side of the calibration report without a GPU: the table, summary and top-label
fold on hand-made rows, `calibration_edges`, the header constants, the entry point's argument checks, the
eval CLI's flags and refusals, the writers, and the temperature fit against an independent minimiser."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import build as B
from selectivenet_for_semantic_segmentation_binary_amd import eval as EV
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT
from tests import _calibration_ref as R

ONE, NAT = 1 << 30, 1 << 20
# k = 4: {non-events, events, sum P, sum B, sum L}
ROWS = [[3, 1, ONE // 2, ONE // 4, NAT],            # 4 pixels at probability 0.125, one event
        [0, 0, 0, 0, 0],                            # empty
        [1, 1, ONE * 5 // 4, ONE // 4, NAT],        # 2 pixels at 0.625, one event
        [0, 2, ONE * 7 // 4, ONE // 2, 2 * NAT]]    # 2 pixels at 0.875, both events


def test_table_on_hand_made_rows():
    t = MT.calibration_table(ROWS, 4)
    assert [r["bin"] for r in t] == [0, 1, 2, 3]
    assert [(r["lo"], r["hi"]) for r in t] == [(0.0, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 1.0)]
    assert [r["n"] for r in t] == [4, 0, 2, 2]
    assert [r["events"] for r in t] == [1, 0, 1, 2] and [r["non_events"] for r in t] == [3, 0, 1, 0]
    assert [r["event_rate"] for r in (t[0], t[2], t[3])] == [0.25, 0.5, 1.0]
    assert [r["mean_score"] for r in (t[0], t[2], t[3])] == [0.125, 0.625, 0.875]
    assert [r["gap"] for r in (t[0], t[2], t[3])] == [0.125, -0.125, 0.125]
    assert all(math.isnan(t[1][c]) for c in ("event_rate", "mean_score", "gap"))
    assert t[3]["sum_score"] == ONE * 7 // 4 and t[3]["sum_brier"] == ONE // 2 and t[3]["sum_nll"] == 2 * NAT
    assert all(set(r) == set(MT.CALIBRATION_BIN_COLUMNS) for r in t)
    with pytest.raises(ValueError):
        MT.calibration_table(ROWS, 6)
    with pytest.raises(ValueError):
        MT.calibration_table(ROWS[:3], 3)


def test_summary_and_fold_on_hand_made_rows():
    s = MT.calibration_summary(ROWS)
    assert s["pixels"] == 8
    assert s["ece"] == 4 / 8 * 0.125 + 2 / 8 * 0.125 + 2 / 8 * 0.125 == 0.125 and s["mce"] == 0.125
    assert s["brier"] == 1 / 8 and s["nll"] == 4 / 8
    top = s["top_label"]
    assert [(r["lo"], r["hi"]) for r in top] == [(0.5, 0.75), (0.75, 1.0)]
    # confidence bin 0 = bin 2 + bin 1 (empty); confidence bin 1 = bin 3 + bin 0
    assert (top[0]["n"], top[0]["correct"], top[0]["sum_confidence"]) == (2, 1, ONE * 5 // 4)
    assert (top[1]["n"], top[1]["correct"], top[1]["sum_confidence"]) == (6, 5, ONE * 7 // 4 + 4 * ONE - ONE // 2)
    assert top[0]["accuracy"] == 0.5 and top[0]["mean_confidence"] == 0.625
    assert top[1]["accuracy"] == 5 / 6 and top[1]["mean_confidence"] == 0.875
    assert s["top_label_ece"] == pytest.approx(2 / 8 * 0.125 + 6 / 8 * (0.875 - 5 / 6), rel=1e-14)
    assert s["top_label_accuracy"] == 6 / 8
    # sums beyond 2^63 (2^33 pixels of 2^30 each) stay exact: Python integers
    big = [[0, 0, 0, 0, 0], [0, 1 << 33, (1 << 63) + 12, 1 << 40, 1 << 40]]
    s = MT.calibration_summary(np.array(big, dtype=object))
    assert s["pixels"] == 1 << 33 and s["top_label"][0]["sum_confidence"] == (1 << 63) + 12 and s["ece"] == 0.0
    empty = MT.calibration_summary(np.zeros((4, 5), np.int64))
    assert empty["pixels"] == 0 and all(math.isnan(empty[c]) for c in ("ece", "mce", "brier", "nll", "top_label_ece",
                                                                        "top_label_accuracy"))
    for bad in (np.zeros((3, 5)), np.zeros((4, 4)), np.zeros(20)):
        with pytest.raises(ValueError):
            MT.calibration_summary(bad)


def test_calibration_edges():
    cuts, thr = MT.calibration_edges(20)
    want_cuts, want = MT.sweep_thresholds([j / 20 for j in range(1, 20)], rule="eval")
    assert cuts == want_cuts == [j / 20 for j in range(1, 20)]
    assert thr.dtype == np.float32 and np.array_equal(thr, want) and len(thr) == 19
    assert float(thr[9]) == MT.logit_threshold("eval", 0.5)
    assert np.all(np.diff(thr) > 0)
    assert len(MT.calibration_edges(2)[1]) == 1 and len(MT.calibration_edges(256)[1]) == 255
    for bad in (3, 19, 0, 1, -2, 258, 257, 2.5, True):
        with pytest.raises(ValueError):
            MT.calibration_edges(bad)
    for bad in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            MT.calibration_edges(20, bad)


def test_calibration_edges_at_a_temperature():
    cuts, thr = MT.calibration_edges(10, 2.0)
    rule = lambda x, c: bool((1 / (1 + np.exp(-(np.array([x], np.float32) / np.float32(2.0))))) > c)  # noqa: E731
    for c, t in zip(cuts, thr):
        assert rule(t, c) and not rule(np.nextafter(t, np.float32(-np.inf)), c)
        assert abs(float(t) - 2.0 * math.log(c / (1 - c))) < 1e-5
    assert np.array_equal(MT.calibration_edges(10, 1.0)[1], MT.calibration_edges(10)[1])


def test_constants_match_the_header():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "selunet.h")
    lines = {ln.split()[1]: ln.split()[2] for ln in open(header) if ln.startswith("#define SELUNET_")
             and len(ln.split()) >= 3}
    for name in ("MAX_EDGES", "FRAC_BITS", "NLL_BITS", "NLL_MAX", "FINE_CELLS"):
        assert int(lines["SELUNET_CALIB_" + name]) == getattr(K, "CALIB_" + name) == getattr(R, name), name
    assert (K.CALIB_MAX_EDGES, K.CALIB_FRAC_BITS, K.CALIB_NLL_BITS, K.CALIB_NLL_MAX, K.CALIB_FINE_CELLS) == \
        (255, 30, 20, 1024, 4098)
    assert K.CALIB_NLL_MAX << K.CALIB_NLL_BITS == 1 << K.CALIB_FRAC_BITS  # every per-pixel word is <= 2^30
    assert (1 << 33) * (1 << K.CALIB_FRAC_BITS) < 1 << 64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(K.lib_path()):
        B.build()
    return K.load()


def test_invalid_arguments_fail_with_a_message(lib):
    """Rejected on the host before any launch: no device is touched (the pointers are host memory)."""
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(score=a, out=a + 512, sel=a + 1024, target=a + 1536, p=16, event=1, t_out=0.0, t_sel=0.0,
              edges=a + 2048, m=3, inv_t=1.0, bins=a + 3072, fine=a + 4096, misc=a + 4608)
    cases = [(dict(score=None), b"null"), (dict(target=None), b"null"), (dict(edges=None), b"null"),
             (dict(bins=None), b"null"), (dict(misc=None), b"null"), (dict(out=None), b"null out"),
             (dict(p=0), b"p must be"), (dict(p=-4), b"p must be"), (dict(p=2 ** 33 + 1), b"p must be"),
             (dict(event=2), b"event"), (dict(event=-1), b"event"),
             (dict(m=0), b"m must be"), (dict(m=256), b"m must be"),
             (dict(inv_t=0.0), b"inv_temperature"), (dict(inv_t=-1.0), b"inv_temperature"),
             (dict(inv_t=float("inf")), b"inv_temperature"), (dict(inv_t=float("nan")), b"inv_temperature"),
             (dict(score=a + 4), b"16-B aligned"), (dict(out=a + 516), b"16-B aligned"),
             (dict(sel=a + 1032), b"16-B aligned"), (dict(target=a + 1540), b"16-B aligned"),
             (dict(edges=a + 2050), b"4-B aligned"), (dict(bins=a + 3076), b"8-B aligned"),
             (dict(fine=a + 4100), b"8-B aligned"), (dict(misc=a + 4612), b"8-B aligned")]
    for kw, part in cases:
        rc = lib.selunet_calibration_bins(*dict(ok, **kw).values(), None)
        msg = lib.selunet_last_error()
        assert rc == 1 and msg and b"calibration_bins" in msg and part in msg, (kw, rc, msg)
    with pytest.raises(RuntimeError):
        K.call("selunet_calibration_bins", *dict(ok, m=300).values(), None)


def test_eval_cli_calibration_flags(capsys, monkeypatch):
    # off: the namespace does not carry the flags at all
    for argv in ([], "--calibration_bins 10 --calibration_temperature 2".split()):
        assert not [k for k in vars(EV.parse_arguments(argv)) if k.startswith("calibration")]
    a = EV.parse_arguments(["--calibration_report", "1"])
    assert a.calibration_report is True and a.calibration_bins == 20 and a.calibration_temperature == 1.0
    a = EV.parse_arguments("--calibration_report 1 --calibration_bins 256 --calibration_temperature 2.5".split())
    assert a.calibration_bins == 256 and a.calibration_temperature == 2.5
    for bad in ("--calibration_bins 19", "--calibration_bins 0", "--calibration_bins 258", "--calibration_bins -2",
                "--calibration_temperature 0", "--calibration_temperature -1", "--calibration_temperature nan",
                "--calibration_temperature inf"):
        with pytest.raises(SystemExit):
            EV.parse_arguments(["--calibration_report", "1"] + bad.split())
        assert "--calibration_" in capsys.readouterr().err
    # the printed args= line: without the report it does not name the three flags, whatever their values
    monkeypatch.setattr(EV, "evaluate", lambda args: None)
    EV.main([])
    plain = capsys.readouterr().out
    EV.main("--calibration_bins 10 --calibration_temperature 2".split())
    assert capsys.readouterr().out == plain and "calibration" not in plain and plain.startswith("\nargs=Namespace(")
    EV.main("--calibration_report 1 --calibration_bins 10".split())
    on = capsys.readouterr().out
    assert on.replace(", calibration_report=True, calibration_bins=10, calibration_temperature=1.0", "") == plain


def test_eval_refuses_outputs_that_are_not_logits(tmp_path):
    """Both refusals come before a device is touched."""
    base = ["--data_dir", "synthetic:8", "--model_dir", str(tmp_path), "--save_dir", str(tmp_path / "out"),
            "--calibration_report", "1"]
    for scale in ("None", "clip", "minmax"):
        with pytest.raises(ValueError, match="single_scale"):
            EV.evaluate(EV.parse_arguments(base + ["--single_scale", scale]))
    for name in ("a.pth", "b.pth"):
        (tmp_path / name).write_bytes(b"")
    for scale in ("sigmoid", "clip", "minmax"):
        with pytest.raises(ValueError, match="ens_scale"):
            EV.evaluate(EV.parse_arguments(base + ["--ens_scale", scale]))
    assert not os.path.exists(tmp_path / "out")


def lossless_case(n=603, t0=2.5, seed=3):
    """Scores on cell midpoints (c + 0.5) / 64, so the fine histogram loses nothing; labels drawn at T0."""
    rng = np.random.Generator(np.random.PCG64(seed))
    score = ((rng.integers(-400, 400, n) + 0.5) / 64).astype(np.float32)
    e = (rng.random(n) < 1 / (1 + np.exp(-score.astype(np.float64) / t0))).astype(np.int64)
    return score, e


def fine_of(score, e):
    return R.calibration_bins(score, None, None, e.astype(np.float32), 0, 0.0, 0.0, [0.0], 1.0)[1]


def test_fit_temperature_on_a_lossless_case():
    score, e = lossless_case()
    fine = fine_of(score, e)
    assert fine.sum() == 603 and np.array_equal(MT.fine_midpoints()[R.fine_cell(score)], score.astype(np.float64))
    for t in (1.0, 2.5, 0.3):
        assert MT.nll_from_fine(fine, t) == pytest.approx(R.exact_nll(score, e, t), rel=1e-12)
    fit = MT.fit_temperature(fine)
    gold = R.golden_temperature(score, e)
    print(f"fit_temperature {fit['temperature']!r}, golden section on the raw scores {gold!r}, relative difference "
          f"{abs(fit['temperature'] - gold) / gold:.3e}")
    assert abs(fit["temperature"] - gold) <= 1e-6 * gold
    assert 1.5 < fit["temperature"] < 4.5  # 603 draws at T0 = 2.5
    assert fit["nll"] == MT.nll_from_fine(fine, 1.0) and fit["nll_fitted"] == MT.nll_from_fine(fine, fit["temperature"])
    assert fit["nll_fitted"] < fit["nll"]
    for t in (fit["temperature"] * 0.99, fit["temperature"] * 1.01):
        assert MT.nll_from_fine(fine, t) > fit["nll_fitted"]


def test_fit_temperature_ends_of_the_range_and_empty():
    fine = np.zeros((K.CALIB_FINE_CELLS, 2), np.int64)
    fit = MT.fit_temperature(fine)
    assert all(math.isnan(v) for v in fit.values()) and math.isnan(MT.nll_from_fine(fine))
    sep = fine.copy()  # separable: the sharper the better
    sep[2049 + 64, 1] = 5
    sep[2049 - 64, 0] = 5
    assert MT.fit_temperature(sep)["temperature"] == 1 / 64
    anti = sep[:, ::-1]  # every score on the wrong side: the flatter the better
    assert MT.fit_temperature(anti)["temperature"] == 64.0
    with pytest.raises(ValueError):
        MT.fit_temperature(np.zeros((4096, 2)))
    x = MT.fine_midpoints()
    assert x[0] == -32 and x[-1] == 32 and x[1] == -32 + 1 / 128 and x[2049] == 1 / 128 and x[4096] == 32 - 1 / 128


def test_nll_from_fine_within_the_midpoint_bound():
    rng = np.random.Generator(np.random.PCG64(4))
    n = 5000
    score = rng.normal(0, 3, n).astype(np.float32)
    assert np.abs(score).max() < 32  # the bound holds only inside the histogram's range
    e = (rng.random(n) < 1 / (1 + np.exp(-score.astype(np.float64) / 1.7))).astype(np.int64)
    got, want = MT.nll_from_fine(fine_of(score, e), 1.0), R.exact_nll(score, e, 1.0)
    print(f"nll_from_fine {got!r}, exact {want!r}: {abs(got - want) * n:.4f} nats over {n} pixels, bound {n / 128}")
    assert abs(got - want) * n <= n / 128


def hand_doc():
    score, e = lossless_case()
    views = {}
    for name, t in (("tumor", 2.0), ("selection", 1.0)):
        views[name] = {"temperature": t, "edge_logits": [0.0] * 3, "nan_scores": 1, "other_labels": 2,
                       "summary": MT.calibration_summary(ROWS), "fit": MT.fit_temperature(fine_of(score, e)),
                       "table": MT.calibration_table(ROWS, 4)}
    return {"bins": 4, "views": views}


def test_report_writers_on_hand_made_rows(tmp_path, capsys):
    doc = hand_doc()
    assert EV.report_calibration(doc, str(tmp_path)) is doc
    text = capsys.readouterr().out.split("\n")
    assert "calibration report (4 bins)" in text[0] and "fitted T" in text[1]
    assert text[2].split()[:6] == ["tumor", "8", "0.125000", "0.062500", "0.125000", "0.125000"]
    assert text[3].split()[0] == "selection" and len(text[2].split()) == 9
    saved = json.load(open(tmp_path / "calibration.json"))
    assert list(saved["views"]) == ["tumor", "selection"] and saved["bins"] == 4
    assert saved["views"]["tumor"]["summary"]["ece"] == 0.125 and saved["views"]["tumor"]["temperature"] == 2.0
    assert saved["views"]["tumor"]["fit"] == doc["views"]["tumor"]["fit"]
    assert saved["views"]["tumor"]["table"][3] == doc["views"]["tumor"]["table"][3]
    lines = open(tmp_path / "calibration_bins.csv").read().strip().split("\n")
    cols = ("view",) + MT.CALIBRATION_BIN_COLUMNS
    assert lines[0].split(",") == list(cols) and len(lines) == 1 + 2 * 4
    for name, at in (("tumor", 1), ("selection", 5)):
        for r, ln in zip(doc["views"][name]["table"], lines[at:at + 4]):
            cells = dict(zip(cols, ln.split(",")))
            assert cells["view"] == name
            for k in MT.CALIBRATION_BIN_COLUMNS:
                assert cells[k] == (repr(r[k]) if isinstance(r[k], float) else str(r[k])), k
    assert lines[1].split(",")[:6] == ["tumor", "0", "0.0", "0.25", "3", "1"]  # integers as integers
    assert lines[2].split(",")[-3:] == ["nan", "nan", "nan"]
