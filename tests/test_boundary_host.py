"""The host side of the boundary-distance metrics without a GPU: the numpy oracle against
scipy and against itself, `band_edges_sq`, the band and patch formulas on hand-made counts, the empty-mask
conventions, the entry points' argument checks, the eval CLI's flags and the writers."""
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
from tests import _boundary_ref as R

INF, NAN = float("inf"), float("nan")


def masks():
    rng = np.random.Generator(np.random.PCG64(5))
    out = [rng.random((h, w)) < p for (h, w) in ((1, 1), (1, 9), (9, 1), (5, 8), (17, 23)) for p in (0.5, 0.05, 0.95)]
    out.append(np.indices((6, 7)).sum(0) % 2 == 0)
    return out


def test_oracle_forms_agree():
    for m in masks():
        a, b = R.brute_d2(m), R.separable_d2(m)
        assert np.array_equal(a, b), (m.shape, a, b)
        one = m.all() or not m.any()
        assert (a == R.NONE).all() if one else (a.min() >= 1 and a.max() < R.NONE)
    assert (R.brute_d2(masks()[-1]) == 1).all()  # checkerboard


def test_oracle_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for m in masks():
        if m.all() or not m.any():
            continue
        want = np.where(m, ndi.distance_transform_edt(m) ** 2, ndi.distance_transform_edt(~m) ** 2)
        assert np.array_equal(R.brute_d2(m), np.rint(want).astype(np.int64)), m.shape


def test_foreground_rule_of_the_oracle():
    x = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nan, np.inf, -np.inf], np.float32)
    assert R.foreground(x, 0.5).tolist() == [True, False, False, True, False]


def test_band_edges_sq():
    r2 = MT.band_edges_sq([1, 2, 4, 8, 16])
    assert r2.dtype == np.float64 and r2.tolist() == [1, 4, 16, 64, 256]
    assert MT.band_edges_sq([1.5, 2.5]).tolist() == [2, 6]
    assert MT.band_edges_sq([1]).tolist() == [1]
    assert len(MT.band_edges_sq(list(range(1, K.BAND_MAX + 1)))) == K.BAND_MAX
    for bad in ([], [0.5, 2], [0], [2, 2], [3, 2], [1, NAN], [1, INF], [2, 2.2],  # floor(2.2^2) == floor(2^2)
                [1.1, 1.2], list(range(1, K.BAND_MAX + 2)), [1, 2.0 ** 16]):
        with pytest.raises(ValueError):
            MT.band_edges_sq(bad)


BINS = [[10, 2, 3, 5, 20, 30],     # band 0
        [40, 1, 0, 9, 50, 50],     # band 1: nothing rejected
        [0, 0, 0, 0, 0, 6],        # band 2: nothing selected
        [0, 0, 0, 0, 0, 0],        # band 3 (beyond the last radius): empty
        [7, 0, 0, 0, 7, 14]]       # no contour


def test_band_table_on_hand_made_counts():
    rows = MT.band_table(BINS, [1, 2.5, 4])
    assert [r["band"] for r in rows] == [0, 1, 2, 3, 4]
    assert [(r["r_lo"], r["r_hi"]) for r in rows[:4]] == [(0.0, 1.0), (1.0, 2.5), (2.5, 4.0), (4.0, INF)]
    assert math.isnan(rows[4]["r_lo"]) and math.isnan(rows[4]["r_hi"])
    assert [r["pixels"] for r in rows] == [30, 50, 6, 0, 14] and [r["selected"] for r in rows] == [20, 50, 0, 0, 7]
    assert [r["pixel_share"] for r in rows] == [30 / 100, 50 / 100, 6 / 100, 0.0, 14 / 100]
    assert [r["errors"] for r in rows] == [5, 1, 0, 0, 0] and [r["rejected"] for r in rows] == [10, 0, 6, 0, 7]
    assert rows[0]["coverage"] == 20 / 30 and rows[0]["risk"] == 5 / 20
    assert rows[1]["coverage"] == 1.0 and rows[1]["risk"] == 1 / 50
    assert rows[2]["coverage"] == 0.0 and math.isnan(rows[2]["risk"])       # nothing selected: no risk
    assert math.isnan(rows[3]["coverage"]) and math.isnan(rows[3]["risk"])  # no pixel: no coverage either
    assert [r["rejected_share"] for r in rows] == [10 / 23, 0.0, 6 / 23, 0.0, 7 / 23]
    assert [r["error_share"] for r in rows] == [5 / 6, 1 / 6, 0.0, 0.0, 0.0]
    assert [r["cum_pixel_share"] for r in rows] == [30 / 100, 80 / 100, 86 / 100, 86 / 100, 1.0]
    assert [r["cum_rejected_share"] for r in rows] == [10 / 23, 10 / 23, 16 / 23, 16 / 23, 1.0]
    assert [r["cum_error_share"] for r in rows] == [5 / 6, 1.0, 1.0, 1.0, 1.0]
    want = R.band_formulas(BINS, [1, 2.5, 4])
    assert all(set(a) == set(MT.BAND_COLUMNS) and all(R.same(a[k], b[k]) for k in a) for a, b in zip(rows, want))
    # nothing rejected and no error anywhere: the shares have no denominator
    rows = MT.band_table([[4, 0, 0, 4, 8, 8], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], [3])
    assert all(math.isnan(r[k]) for r in rows for k in ("rejected_share", "error_share", "cum_error_share"))
    assert rows[0]["risk"] == 0.0 and rows[0]["cum_pixel_share"] == 1.0
    with pytest.raises(ValueError):
        MT.band_table(BINS, [1, 2])


def test_boundary_patch_on_hand_made_counts():
    # cm = [tn, fp, fn, tp]; words = [fp max d2, fn max d2, fp within, fn within, fp, fn]
    r = MT.boundary_patch([25, 2, 3, 1, 5, 2], [80, 5, 2, 13, 100, 100])
    assert r["hd_pred_to_label"] == 5.0 and r["hd_label_to_pred"] == math.sqrt(2) and r["hausdorff"] == 5.0
    assert r["tolerant_accuracy"] == (13 + 80 + 4) / 100 and r["tolerant_tumor_iou"] == (13 + 4) / 20
    assert [r[k] for k in MT.BOUNDARY_WORDS] == [25, 2, 3, 1, 5, 2]
    assert all(R.same(r[k], v) for k, v in R.patch_formulas([25, 2, 3, 1, 5, 2], [80, 5, 2, 13]).items())
    # no error at all: distance 0, scores 1
    r = MT.boundary_patch([0, 0, 0, 0, 0, 0], [90, 0, 0, 10, 100, 100])
    assert (r["hausdorff"], r["hd_pred_to_label"], r["hd_label_to_pred"]) == (0.0, 0.0, 0.0)
    assert r["tolerant_accuracy"] == 1.0 and r["tolerant_tumor_iou"] == 1.0
    # prefix, and counts that contradict the words
    assert set(MT.boundary_patch([0] * 6, [1, 0, 0, 1, 2, 2], prefix="sel_")) == {
        "sel_" + k for k in MT.BOUNDARY_WORDS + MT.BOUNDARY_METRICS}
    with pytest.raises(ValueError):
        MT.boundary_patch([4, 0, 0, 0, 1, 0], [9, 2, 0, 1, 12, 12])


def test_empty_mask_conventions():
    none = K.EDT_NONE
    assert none == R.NONE == 2 ** 31 - 1
    # empty label, a prediction: every false positive is infinitely far from the label region
    r = MT.boundary_patch([none, 0, 0, 0, 7, 0], [93, 7, 0, 0, 100, 100])
    assert r["hd_pred_to_label"] == INF and r["hd_label_to_pred"] == 0.0 and r["hausdorff"] == INF
    assert r["tolerant_accuracy"] == 0.93 and r["tolerant_tumor_iou"] == 0.0
    # empty prediction, a label: the converse
    r = MT.boundary_patch([0, none, 0, 0, 0, 4], [96, 0, 4, 0, 100, 100])
    assert r["hd_pred_to_label"] == 0.0 and r["hd_label_to_pred"] == INF and r["hausdorff"] == INF
    # both empty: no error, distance 0; the tumor IoU has no denominator
    r = MT.boundary_patch([0] * 6, [100, 0, 0, 0, 100, 100])
    assert r["hausdorff"] == 0.0 and r["tolerant_accuracy"] == 1.0 and math.isnan(r["tolerant_tumor_iou"])
    # nothing selected: no counted pixel
    r = MT.boundary_patch([0] * 6, [0, 0, 0, 0, 0, 100])
    assert r["hausdorff"] == 0.0 and math.isnan(r["tolerant_accuracy"])
    # the summary keeps the infinite rows out of the mean
    rows = [{"hausdorff": v} for v in (INF, 0.0, 3.0, 5.0, 0.0)]
    doc = MT.boundary_report_summary(rows)
    assert doc == {"patches": 5, "infinite_hausdorff": 1, "zero_hausdorff": 2, "mean_hausdorff": 2.0,
                   "median_hausdorff": 1.5}
    doc = MT.boundary_report_summary([{"hausdorff": INF}])
    assert doc["infinite_hausdorff"] == 1 and math.isnan(doc["mean_hausdorff"]) and math.isnan(doc["median_hausdorff"])
    doc = MT.boundary_report_summary([])
    assert doc["patches"] == 0 and doc["infinite_hausdorff"] == 0 and math.isnan(doc["mean_hausdorff"])


def test_constants_match_the_header():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "selunet.h")
    lines = {ln.split()[1]: ln.split()[2] for ln in open(header) if ln.startswith("#define SELUNET_")
             and len(ln.split()) >= 3}
    assert lines["SELUNET_EDT_NONE"] == "INT32_MAX"
    assert int(lines["SELUNET_EDT_MAX_SIDE"]) == K.EDT_MAX_SIDE and int(lines["SELUNET_BAND_MAX"]) == K.BAND_MAX
    assert 2 * (K.EDT_MAX_SIDE - 1) ** 2 < K.EDT_NONE


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(K.lib_path()):
        B.build()
    return K.load()


def test_invalid_arguments_fail_with_a_message(lib):
    """Rejected on the host before any launch: no device is touched (the pointers are host memory)."""
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 15) & ~15
    r2 = (ctypes.c_int32 * 16)(*range(1, 17))

    def rejected(fn, args, part):
        rc = getattr(lib, fn)(*args, None)
        msg = lib.selunet_last_error()
        assert rc == 1 and msg and fn[len("selunet_"):].encode() in msg and part in msg, (fn, args, rc, msg)

    edt = dict(x=a, t=0.5, n=2, h=4, w=4, d2=a + 1024)
    for kw, part in ((dict(x=None), b"null"), (dict(d2=None), b"null"), (dict(n=0), b"n must be"),
                     (dict(h=0), b"h and w"), (dict(w=4097), b"h and w"), (dict(h=4097), b"h and w"),
                     (dict(n=2 ** 20, h=4096), b"2^31"), (dict(x=a + 2), b"4-B aligned")):
        rejected("selunet_edt_sq", list(dict(edt, **kw).values()), part)
    bands = dict(out=a, sel=a + 1024, target=a + 2048, d2=a + 3072, n=2, hw=16, t_out=0.0, t_sel=0.0, r2=r2, k=3,
                 bins=a + 4096)
    for kw, part in ((dict(out=None), b"null"), (dict(d2=None), b"null"), (dict(bins=None), b"null"),
                     (dict(r2=None), b"null"), (dict(n=0), b"n and hw"), (dict(hw=0), b"n and hw"),
                     (dict(n=2 ** 20, hw=2 ** 21), b"n and hw"), (dict(k=0), b"k must be"), (dict(k=16), b"k must be"),
                     (dict(r2=(ctypes.c_int32 * 3)(0, 1, 2)), b"strictly increasing"),
                     (dict(r2=(ctypes.c_int32 * 3)(1, 4, 4)), b"strictly increasing"),
                     (dict(r2=(ctypes.c_int32 * 3)(4, 2, 9)), b"strictly increasing"),
                     (dict(sel=a + 1028), b"16-B aligned"), (dict(d2=a + 3076), b"16-B aligned"),
                     (dict(bins=a + 4100), b"8-B aligned")):
        rejected("selunet_boundary_bands", list(dict(bands, **kw).values()), part)
    rows = dict(out=a, sel=a + 1024, target=a + 2048, d2t=a + 3072, d2p=a + 4096, n=2, hw=16, t_out=0.0, t_sel=0.0,
                tol=4, rows=a + 5120)
    for kw, part in ((dict(out=None), b"null"), (dict(d2p=None), b"null"), (dict(rows=None), b"null"),
                     (dict(n=0), b"n must be"), (dict(hw=0), b"hw must be"), (dict(hw=2 ** 24 + 1), b"hw must be"),
                     (dict(tol=-1), b"tol_sq"), (dict(d2t=a + 3076), b"16-B aligned"),
                     (dict(hw=15, sel=a + 1026), b"aligned"), (dict(rows=a + 5124), b"8-B aligned")):
        rejected("selunet_boundary_rows", list(dict(rows, **kw).values()), part)
    with pytest.raises(RuntimeError):
        K.call("selunet_edt_sq", a, 0.5, 1, 4097, 4, a + 1024, None)


def test_eval_cli_boundary_flags(capsys, monkeypatch):
    # off: the namespace does not carry the flags at all (whoever prints or copies it sees what it was before)
    for argv in ([], "--boundary_bands 3 5 --boundary_tolerance 1".split()):
        assert not [k for k in vars(EV.parse_arguments(argv)) if k.startswith("boundary")]
    a = EV.parse_arguments(["--boundary_report", "1"])
    assert a.boundary_report is True and a.boundary_bands == [1, 2, 4, 8, 16] and a.boundary_tolerance == 2
    a = EV.parse_arguments(
        "--boundary_report 1 --boundary_bands 1.5 3 6 --boundary_tolerance 0 --patch_report 1".split())
    assert a.boundary_report is True and a.boundary_bands == [1.5, 3.0, 6.0] and a.boundary_tolerance == 0.0
    assert a.patch_report is True
    for bad in ("--boundary_report 1 --boundary_bands 2 2", "--boundary_report 1 --boundary_bands 0.5",
                "--boundary_report 1 --boundary_bands 2 2.2", "--boundary_report 1 --boundary_tolerance -1",
                "--boundary_report 1 --boundary_tolerance nan",
                "--boundary_report 1 --boundary_bands " + " ".join(str(i) for i in range(1, 18))):
        with pytest.raises(SystemExit):
            EV.parse_arguments(bad.split())
        assert "--boundary_" in capsys.readouterr().err
    # the printed args= line: without the report it does not name the three flags, whatever their values
    monkeypatch.setattr(EV, "evaluate", lambda args: None)
    EV.main([])
    plain = capsys.readouterr().out
    EV.main("--boundary_bands 3 5 --boundary_tolerance 1".split())
    assert capsys.readouterr().out == plain and "boundary" not in plain and plain.startswith("\nargs=Namespace(")
    EV.main("--boundary_report 1 --boundary_bands 3 5".split())
    on = capsys.readouterr().out
    assert "boundary_report=True" in on and "boundary_bands=[3.0, 5.0]" in on and "boundary_tolerance=2" in on
    assert on.replace(", boundary_report=True, boundary_bands=[3.0, 5.0], boundary_tolerance=2", "") == plain


def hand_rows(selective):
    data = [([25, 2, 3, 1, 5, 2], [80, 5, 2, 13, 100, 100], [9, 0, 1, 0, 1, 0], [40, 1, 0, 9, 50, 100]),
            ([K.EDT_NONE, 0, 0, 0, 7, 0], [93, 7, 0, 0, 100, 100], [0] * 6, [0, 0, 0, 0, 0, 100]),
            ([0] * 6, [100, 0, 0, 0, 100, 100], [0] * 6, [60, 0, 0, 0, 60, 100])]
    rows = []
    for i, (w, c, sw, sc) in enumerate(data):
        row = {"index": i, "id": ["slideA_0_256", None, "slideB_512_0"][i] or f"patch_{i}", "pixels": c[5]}
        row.update(MT.boundary_patch(w, c))
        if selective:
            row["selected"] = sc[4]
            row.update(MT.boundary_patch(sw, sc, prefix="sel_"))
        rows.append(row)
    return rows


@pytest.mark.parametrize("selective", [False, True])
def test_report_writers_on_hand_made_rows(tmp_path, capsys, selective):
    rows, bands = hand_rows(selective), MT.band_table(BINS, [1, 2.5, 4])
    doc = EV.report_boundary(bands, rows, [1, 2.5, 4], 2.0, str(tmp_path))
    text = capsys.readouterr().out
    assert "boundary report:" in text and "1 < d <= 2.5" in text and "d > 4" in text and "no contour" in text
    assert "Hausdorff distance over 3 patches: mean 2.500000 median 2.500000 (1 infinite, 1 zero)" in text
    assert doc["rows"] is rows and doc["bands"] is bands and doc["tolerance"] == 2.0
    saved = json.load(open(tmp_path / "patch_boundary.json"))
    assert saved == {k: v for k, v in doc.items() if k not in ("rows", "bands")}
    assert saved["patches"] == 3 and saved["infinite_hausdorff"] == 1 and saved["zero_hausdorff"] == 1
    assert ("sel_mean_hausdorff" in saved) == selective
    if selective:
        assert saved["sel_zero_hausdorff"] == 2 and saved["sel_mean_hausdorff"] == 1.0
    lines = open(tmp_path / "patch_boundary.csv").read().strip().split("\n")
    cols = MT.boundary_report_columns(rows)
    assert lines[0].split(",") == list(cols) and len(lines) == 4
    assert ("sel_hausdorff" in cols) == selective and cols[:3] == ("index", "id", "pixels")
    for r, ln in zip(rows, lines[1:]):
        cells = dict(zip(cols, ln.split(",")))
        for k in cols:
            assert cells[k] == (repr(r[k]) if isinstance(r[k], float) else str(r[k])), k
    assert lines[1].split(",")[:5] == ["0", "slideA_0_256", "100", "25", "2"]  # integers as integers
    assert "inf" in lines[2].split(",") and str(K.EDT_NONE) in lines[2].split(",")
    assert float(dict(zip(cols, lines[1].split(",")))["hd_label_to_pred"]) == math.sqrt(2)  # repr round-trips
    lines = open(tmp_path / "boundary_bands.csv").read().strip().split("\n")
    assert lines[0].split(",") == list(MT.BAND_COLUMNS) and len(lines) == 6
    for r, ln in zip(bands, lines[1:]):
        cells = dict(zip(MT.BAND_COLUMNS, ln.split(",")))
        for k in MT.BAND_COLUMNS:
            assert cells[k] == (repr(r[k]) if isinstance(r[k], float) else str(r[k])), k
    saved = json.load(open(tmp_path / "boundary_bands.json"))
    assert saved["radii"] == [1, 2.5, 4] and len(saved["bands"]) == 5
    assert all(R.same(a[k], b[k]) for a, b in zip(saved["bands"], bands) for k in b)
