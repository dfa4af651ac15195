"""The calibration report on the GPU: `selunet_calibration_bins` against the numpy reference
(counts, the fine histogram and misc bit-exact; the fixed-point sums within one unit per pixel) and against
`selunet_seg_metrics`, `metrics.CalibrationReport`, and the eval CLI's --calibration_report against the CPU
oracle.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import eval as EV
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT
from tests import _calibration_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
T_OUT = F32(MT.logit_threshold("eval", 0.5))
T_SEL = F32(MT.logit_threshold("eval", 0.4))
ONE = 1 << 30


# ----------------------------------------------------------------------------- kernel level
def run_calib(score, out, sel, tgt, event, edges, inv_t=1.0, calls=1, fine=True, t_out=T_OUT, t_sel=T_SEL):
    """(bins [(m+1)][5], fine [4098][2] or None, misc [2]) of `calls` accumulating kernel calls."""
    dev = [a if a is None or torch.is_tensor(a) else torch.tensor(a, device=DEV) for a in (score, out, sel, tgt)]
    ed = torch.tensor(np.asarray(edges, F32), device=DEV)
    bins = torch.zeros(len(edges) + 1, 5, dtype=torch.int64, device=DEV)
    hist = torch.zeros(K.CALIB_FINE_CELLS, 2, dtype=torch.int64, device=DEV) if fine else None
    misc = torch.zeros(2, dtype=torch.int64, device=DEV)
    for _ in range(calls):
        K.call("selunet_calibration_bins", K.ptr(dev[0]), K.ptr(dev[1]), K.ptr(dev[2]), K.ptr(dev[3]), dev[0].numel(),
               event, float(t_out), float(t_sel), K.ptr(ed), len(edges), float(inv_t), K.ptr(bins), K.ptr(hist),
               K.ptr(misc), K.stream_ptr())
    return bins.cpu().numpy(), None if hist is None else hist.cpu().numpy(), misc.cpu().numpy()


def edge_case(edges, seed):
    """As test_gpu_sweep.edge_case: a ragged tail (p = 4*3*50*r + 3, r = 1 unless the edge values need more), and
    in `score` every edge and its two fp32 neighbours, +-0, +-inf, nan, +-40, the fine histogram's cell
    boundaries +-32 and j/64 with their neighbours; the thresholds of `out` and `sel` with theirs; a few
    labels >= 2."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def around(v):
        v = np.asarray(v, F32)
        with np.errstate(invalid="ignore"):
            return np.concatenate([v, np.nextafter(v, F32(-np.inf)), np.nextafter(v, F32(np.inf))]).astype(F32)

    special = np.array([0, -0.0, np.inf, -np.inf, np.nan, 40, -40], F32)
    cells = np.array([32, -32] + [j / 64 for j in (-2048, -2047, -65, -1, 1, 2, 64, 777, 2047)], F32)
    edge = np.concatenate([around(edges), special, around(cells)])
    other = np.concatenate([around([T_OUT, T_SEL]), special])
    r = 1
    while 4 * 3 * 50 * r + 3 < 2 * len(edge) + 5:
        r += 1
    p = 4 * 3 * 50 * r + 3
    score = rng.normal(0, 2.5, p).astype(F32)
    out = rng.normal(0, 1, p).astype(F32)
    sel = rng.normal(0, 1, p).astype(F32)
    score[:len(edge)] = edge
    score[-len(edge):] = edge[::-1]  # the ragged tail sees edge values too
    out[3:3 + len(other)] = other
    sel[7:7 + len(other)] = other
    out[-len(other):] = other
    sel[-len(other) - 2:-2] = other[::-1]
    tgt = (rng.random(p) > 0.4).astype(F32)
    tgt[rng.choice(p, 9, replace=False)] = np.array([2, 255, 2, 255, 2, 255, 2, 255, 2], F32)
    return score, out, sel, tgt


M_CASES = {1: 2, 19: 20, 255: 256}  # m edges -> k bins
INV_T = (1.0, 0.4, 2.0)


@functools.lru_cache(maxsize=None)
def kernel_case(m, inv_t):
    """Every (event, sel, calls) combination of one (m, inv_temperature): [(key, got, want, calls)]."""
    _, edges = MT.calibration_edges(M_CASES[m], 1.0 / inv_t)
    assert len(edges) == m and np.all(edges[1:] >= edges[:-1])
    score, out, sel, tgt = edge_case(edges, seed=21 + m)
    assert score.size % 4 == 3 and (score.size == 603 or m == 255)
    runs = []
    for event in (0, 1):
        for use_sel in (False, True):
            want = R.calibration_bins(score, out, sel if use_sel else None, tgt, event, T_OUT, T_SEL, edges, inv_t)
            for calls in (1, 2):
                got = run_calib(score, out if event else None, sel if use_sel else None, tgt, event, edges, inv_t, calls)
                runs.append(((event, use_sel, calls), got, want, calls))
    return runs


@pytest.mark.parametrize("inv_t", INV_T)
@pytest.mark.parametrize("m", list(M_CASES))
def test_kernel_counts_bit_exact_against_numpy(m, inv_t):
    for key, (bins, fine, misc), (wb, wf, wm), calls in kernel_case(m, inv_t):
        assert bins.shape == (m + 1, 5) and (bins >= 0).all()
        assert wm[1] > 0 and (key[1] or wm[0] > 0) and wb[:, :2].sum() > 300  # the case is not degenerate
        assert np.count_nonzero(wb[:, :2].sum(1)) >= min(m + 1, 20) and (wb[:, :2].sum(0) > 0).all(), key
        assert wf[0].sum() > 0 and wf[-1].sum() > 0 and np.count_nonzero(wf) > 100
        assert np.array_equal(bins[:, :2], calls * wb[:, :2]), key
        assert np.array_equal(fine, calls * wf), key
        assert np.array_equal(misc, calls * wm), key
        assert fine.sum() == bins[:, :2].sum()


@pytest.mark.parametrize("inv_t", INV_T)
@pytest.mark.parametrize("m", list(M_CASES))
def test_kernel_sums_within_a_unit_per_pixel(m, inv_t):
    """Both sides evaluate the same fp64 expression with library functions good to about an ulp (2^-52 relative,
    far below a unit of 2^-30 / 2^-20), so they can differ only where a rounding tie falls differently: by at
    most one unit per pixel, n_b per bin."""
    worst = 0
    for key, (bins, _, _), (wb, _, _), calls in kernel_case(m, inv_t):
        n = bins[:, 0] + bins[:, 1]
        d = np.abs(bins[:, 2:] - calls * wb[:, 2:])
        worst = max(worst, int(d.max()))
        assert (d <= n[:, None]).all(), (key, d.max())
        assert wb[:, 2].sum() > 4 * ONE and (wb[:, 3:].sum(0) > 0).all()  # the sum of P is past 32 bits
    print(f"m = {m}, inv_temperature = {inv_t}: the largest difference of a bin's sum from numpy's is {worst} units")


def test_kernel_without_a_fine_histogram():
    _, edges = MT.calibration_edges(20)
    score, out, sel, tgt = edge_case(edges, seed=5)
    a = run_calib(score, None, sel, tgt, 0, edges, fine=True)
    b = run_calib(score, None, sel, tgt, 0, edges, fine=False)
    assert b[1] is None and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


def seg_counts(out, sel, tgt, t_out=T_OUT, t_sel=T_SEL):
    counts = torch.zeros(6, dtype=torch.int64, device=DEV)
    K.call("selunet_seg_metrics", K.ptr(out), K.ptr(sel), K.ptr(tgt), out.numel(), float(t_out), float(t_sel),
           K.ptr(counts), K.stream_ptr())
    return counts.cpu().numpy()


@pytest.mark.parametrize("use_sel", [False, True])
def test_kernel_against_seg_metrics(use_sel):
    """With the 19 eval-rule edges the middle edge is the Evaluator's prediction threshold."""
    _, edges = MT.calibration_edges(20)
    assert F32(edges[9]) == T_OUT
    score, out, sel, tgt = edge_case(edges, seed=31)
    score[np.isnan(score)] = F32(0.25)  # seg_metrics counts a NaN as background, the report leaves it out
    st, ot, lt, tt = (torch.tensor(a, device=DEV) for a in (score, out, sel, tgt))
    sl = lt if use_sel else None
    bins, _, misc = run_calib(st, None, sl, tt, 0, edges)
    c = seg_counts(st, sl, tt)
    assert misc[0] == 0 and c[:4].min() > 0
    assert bins[10:, 0].sum() == c[1] and bins[10:, 1].sum() == c[3]  # cm[0][1], cm[1][1]
    assert bins[:10, 0].sum() == c[0] and bins[:10, 1].sum() == c[2]  # cm[0][0], cm[1][0]
    assert bins[:, :2].sum() + misc[1] == c[4]
    bins, _, misc = run_calib(st, ot, sl, tt, 1, edges)  # the event: `out` is right
    c = seg_counts(ot, sl, tt)
    assert bins[:, 1].sum() == c[0] + c[3] and bins[:, 0].sum() == c[1] + c[2]


# 16 x 256 x 256 + 3 pixels: the grid is capped at 256 workgroups of 256 threads x 4 pixels, so every workgroup
# makes four stride passes, plus the tail
P_BIG = 16 * 256 * 256 + 3
EDGES_BIG = np.linspace(-4, 4, 101).astype(F32)


@pytest.fixture(scope="module")
def big():
    rng = np.random.Generator(np.random.PCG64(13))
    out = rng.normal(0, 1, P_BIG).astype(F32)
    tgt = (rng.random(P_BIG) > 0.4).astype(F32)
    tgt[rng.choice(P_BIG, 1000, replace=False)] = 2.0
    return {"out": out, "tgt": tgt, "out_d": torch.tensor(out, device=DEV), "tgt_d": torch.tensor(tgt, device=DEV)}


def assert_same(got, want, what):
    (bins, fine, misc), (wb, wf, wm) = got, want
    assert np.array_equal(bins[:, :2], wb[:, :2]), what
    assert np.array_equal(fine, wf) and np.array_equal(misc, wm), what
    d = np.abs(bins[:, 2:] - wb[:, 2:])
    assert (d <= (wb[:, 0] + wb[:, 1])[:, None]).all(), (what, d.max())
    return int(d.max())


def test_kernel_many_workgroups_uniform_bins(big):
    rng = np.random.Generator(np.random.PCG64(14))
    score = rng.uniform(-4.08, 4.08, P_BIG).astype(F32)  # 102 bins of width 0.08
    for event, inv_t in ((0, 1.0), (1, 0.5)):
        want = R.calibration_bins(score, big["out"], None, big["tgt"], event, T_OUT, T_SEL, EDGES_BIG, inv_t)
        assert (want[0][:, :2].sum(1) > P_BIG // 102 // 2).all() and want[2][1] == 1000
        got = run_calib(torch.tensor(score, device=DEV), big["out_d"], None, big["tgt_d"], event, EDGES_BIG, inv_t)
        worst = assert_same(got, want, event)
        assert got[0][:, :2].sum() == P_BIG - 1000
        print(f"event {event}: the largest difference of a bin's sum from numpy's over {P_BIG} pixels is {worst} units")


@pytest.mark.parametrize("value,bin_,cell", [(np.inf, 101, 4097), (-np.inf, 0, 0), (40.0, 101, 4097)])
def test_kernel_every_pixel_in_one_bin(big, value, bin_, cell):
    """Maximum contention on one bin and one cell: a narrow on-chip sum or a lost update shows here."""
    score = np.full(P_BIG, value, F32)
    want = R.calibration_bins(score, None, None, big["tgt"], 0, T_OUT, T_SEL, EDGES_BIG, 1.0)
    got = run_calib(torch.tensor(score, device=DEV), None, None, big["tgt_d"], 0, EDGES_BIG)
    assert_same(got, want, value)
    bins, fine, misc = got
    n0, n1 = int(bins[bin_, 0]), int(bins[bin_, 1])
    assert n0 + n1 == P_BIG - 1000 and misc.tolist() == [0, 1000] and min(n0, n1) > P_BIG // 4
    assert np.count_nonzero(bins[:, :2].sum(1)) == 1 and np.count_nonzero(fine.sum(1)) == 1
    assert fine[cell].tolist() == [n0, n1]
    # sigmoid(+inf) = 1, sigmoid(-inf) = 0 and sigmoid(40) rounds to 1 in fp64
    assert int(bins[bin_, 2]) == (0 if value < 0 else (n0 + n1) * ONE)
    n_wrong = n1 if value < 0 else n0
    assert int(bins[bin_, 3]) == n_wrong * ONE  # (s - e)^2 = 1 for the wrong ones, 0 for the others
    if np.isinf(value):  # the capped 1024 nats = 2^30 units for each wrong pixel, nothing for a right one
        assert int(bins[bin_, 4]) == n_wrong * ONE


# ----------------------------------------------------------------------------- CalibrationReport
def test_calibration_report_class():
    rng = np.random.Generator(np.random.PCG64(15))
    out, sel = (rng.normal(0, 2, (2, 5, 7)).astype(F32) for _ in range(2))
    tgt = (rng.random((2, 5, 7)) > 0.5).astype(F32)
    out[0, 0, 0], sel[0, 0, 1], tgt[1, 0, 0] = np.nan, np.nan, 2
    ot, st, tt = (torch.tensor(a, device=DEV) for a in (out, sel, tgt))
    rep = MT.CalibrationReport(DEV, selective=True, select_eval=True, bins=10, temperature=1.5, s_cut_off=0.4)
    assert rep.views == ["tumor", "tumor_selected", "selection"]
    assert MT.CalibrationReport(DEV, selective=False, select_eval=False).views == ["tumor"]
    assert MT.CalibrationReport(DEV, selective=True, select_eval=False).views == ["tumor", "selection"]
    rep.add_batch(ot, tt, st)
    rep.add_batch(ot, tt, st)
    raw = rep.raw()
    e_t, e_s = MT.calibration_edges(10, 1.5)[1], MT.calibration_edges(10)[1]
    want = {"tumor": R.calibration_bins(out, None, None, tgt, 0, T_OUT, T_SEL, e_t, 1 / 1.5),
            "tumor_selected": R.calibration_bins(out, None, sel, tgt, 0, T_OUT, T_SEL, e_t, 1 / 1.5),
            "selection": R.calibration_bins(sel, out, None, tgt, 1, T_OUT, T_SEL, e_s, 1.0)}
    assert list(raw) == rep.views
    for view in rep.views:
        got = (raw[view]["bins"], raw[view]["fine"], raw[view]["misc"])
        assert got[0].shape == (10, 5) and got[0].dtype == np.int64
        assert_same(got, tuple(2 * w for w in want[view]), view)
    assert raw["tumor"]["misc"].tolist() == [2, 2] and raw["selection"]["misc"].tolist() == [2, 2]
    assert raw["tumor"]["bins"][:, :2].sum() == 2 * 68 and 0 < raw["tumor_selected"]["bins"][:, :2].sum() < 2 * 68
    doc = rep.report()
    assert doc["bins"] == 10 and list(doc["views"]) == rep.views
    for view in rep.views:
        v = doc["views"][view]
        assert v["temperature"] == (1.0 if view == "selection" else 1.5)
        assert json.dumps(v["summary"]) == json.dumps(MT.calibration_summary(raw[view]["bins"]))  # NaNs compare equal
        assert v["fit"] == MT.fit_temperature(raw[view]["fine"]) and len(v["table"]) == 10 and len(v["edge_logits"]) == 9
        assert [v["nan_scores"], v["other_labels"]] == raw[view]["misc"].tolist()
    rep.reset()
    assert not any(r[k].any() for r in rep.raw().values() for k in r)
    for bad in ((ot.transpose(1, 2), tt, st), (ot, tt, st.transpose(1, 2)), (ot.double(), tt, st),
                (ot, tt.to(torch.int64), st), (ot.cpu(), tt, st)):
        with pytest.raises(RuntimeError):
            rep.add_batch(*bad)
    for bad in ((ot[:1].contiguous(), tt, st), (ot, tt, st[:1].contiguous()), (ot, tt, None)):
        with pytest.raises(ValueError):
            rep.add_batch(*bad)
    assert not any(r[k].any() for r in rep.raw().values() for k in r)
    for kw in (dict(bins=7), dict(bins=258), dict(temperature=0.0), dict(selective=False, select_eval=True)):
        with pytest.raises(ValueError):
            MT.CalibrationReport(DEV, **dict(dict(selective=True, select_eval=True), **kw))


# ----------------------------------------------------------------------------- eval CLI
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("calibration_cli")
    ck = tmp / "checkpoint"
    ck.mkdir()
    o, s, lab = R.calibrated_checkpoint(ck / "model_epoch1.pth")
    base = ["--data_dir", "synthetic:8", "--patch_size", "64", "--test_fold", "2", "--model_dir", str(ck),
            "--model_arch", "UNet_B", "--selective", "1", "--batch_size", "4"]

    def run(name, *extra):
        out = tmp / name
        res = EV.evaluate(EV.parse_arguments(base + ["--save_dir", str(out)] + list(extra)))
        return res, out

    on, on_dir = run("on", "--select_eval", "1", "--calibration_report", "1")
    _, off_dir = run("off", "--select_eval", "1")
    _, all_dir = run("all", "--calibration_report", "1")
    t_fit = on["calibration_report"]["views"]["tumor"]["fit"]["temperature"]
    _, fit_dir = run("fitted", "--select_eval", "1", "--calibration_report", "1", "--calibration_temperature", repr(t_fit))
    return {"o": o, "s": s, "lab": lab, "on": on, "on_dir": on_dir, "off_dir": off_dir, "all_dir": all_dir,
            "fit_dir": fit_dir, "t_fit": t_fit}


def oracle_views(c):
    t = F32(MT.logit_threshold("eval", 0.5))
    edges = MT.calibration_edges(20)[1]
    return {"tumor": R.calibration_bins(c["o"], None, None, c["lab"], 0, t, t, edges, 1.0),
            "tumor_selected": R.calibration_bins(c["o"], None, c["s"], c["lab"], 0, t, t, edges, 1.0),
            "selection": R.calibration_bins(c["s"], c["o"], None, c["lab"], 1, t, t, edges, 1.0)}


def file_rows(view):
    return np.array([[r["non_events"], r["events"], r["sum_score"], r["sum_brier"], r["sum_nll"]]
                     for r in view["table"]], np.int64)


def test_eval_cli_calibration_oracle_preconditions(cli):
    """On the oracle alone, so the comparison below cannot pass vacuously."""
    views = oracle_views(cli)
    for name, (bins, _, misc) in views.items():
        n = bins[:, 0] + bins[:, 1]
        both = int(((bins[:, 0] > 0) & (bins[:, 1] > 0)).sum())
        print(f"{name}: {np.count_nonzero(n)} of 20 bins hold pixels, {both} hold both events, {n.sum()} pixels")
        assert np.count_nonzero(n) >= 8 and both >= 5 and not misc.any(), name
    sel = views["tumor_selected"][0][:, :2].sum()
    assert 0.25 * cli["lab"].size < sel < 0.75 * cli["lab"].size
    assert max(np.abs(cli["o"]).max(), np.abs(cli["s"]).max()) < 32  # inside the fine histogram's range


def test_eval_cli_calibration_matches_oracle(cli):
    """<= 1e-3 of the pixels may differ above each edge: those whose logit lies within fp32 rounding of a
    threshold (the cap of test_gpu_sweep.test_eval_cli_sweep_rows_match_oracle on this checkpoint)."""
    doc = json.load(open(cli["on_dir"] / "calibration.json"))
    assert list(doc["views"]) == ["tumor", "tumor_selected", "selection"] and doc["bins"] == 20
    n = cli["lab"].size
    for name, (want, _, _) in oracle_views(cli).items():
        got = file_rows(doc["views"][name])
        above = lambda b: np.cumsum(b[::-1, :2], axis=0)[::-1][1:]  # noqa: E731  row j: the bins above edge j
        d = np.abs(above(got) - above(want)).sum(1)
        print(f"{name}: per edge, the counts above it differ from the oracle's by {d.tolist()} of {n} pixels")
        assert len(d) == 19 and (d <= 1e-3 * n).all(), (name, d)


def test_eval_cli_calibration_invariants(cli):
    doc = json.load(open(cli["on_dir"] / "calibration.json"))
    n = cli["lab"].size
    for name, v in doc["views"].items():
        assert sum(r["n"] for r in v["table"]) == v["summary"]["pixels"], name
        assert sum(r["n"] for r in v["summary"]["top_label"]) == v["summary"]["pixels"], name
        assert v["nan_scores"] == 0 and v["other_labels"] == 0
    assert doc["views"]["tumor"]["summary"]["pixels"] == doc["views"]["selection"]["summary"]["pixels"] == n
    perf = json.load(open(cli["on_dir"] / "performance.json"))
    assert (n - doc["views"]["tumor_selected"]["summary"]["pixels"]) / n == perf["rejection_ratio"]
    assert doc["views"]["tumor_selected"]["summary"]["top_label_accuracy"] == perf["Acc"]  # over the selected pixels
    # without --select_eval: two views, and the top-label accuracy of all pixels is the Evaluator's
    full = json.load(open(cli["all_dir"] / "calibration.json"))
    assert list(full["views"]) == ["tumor", "selection"]
    assert full["views"]["tumor"]["summary"]["top_label_accuracy"] == \
        json.load(open(cli["all_dir"] / "performance.json"))["Acc"]
    for name in ("tumor", "selection"):  # the same counts whatever --select_eval
        assert np.array_equal(file_rows(full["views"][name])[:, :2], file_rows(doc["views"][name])[:, :2]), name
    lines = open(cli["on_dir"] / "calibration_bins.csv").read().strip().split("\n")
    assert lines[0].split(",")[:2] == ["view", "bin"] and len(lines) == 1 + 3 * 20
    assert json.dumps(cli["on"]["calibration_report"]) == json.dumps(doc)  # what evaluate returns is what it wrote


def test_eval_cli_calibration_at_the_fitted_temperature(cli):
    """A midpoint of the fine histogram is within 1/128 of its score and softplus is 1-Lipschitz: the exact
    mean NLL at T is within 1 / (128 T) of the histogram's (N / (128 T) nats over the N pixels)."""
    first = json.load(open(cli["on_dir"] / "calibration.json"))["views"]["tumor"]
    second = json.load(open(cli["fit_dir"] / "calibration.json"))["views"]["tumor"]
    t = cli["t_fit"]
    assert first["fit"]["temperature"] == t and second["temperature"] == t and 1 / 64 <= t <= 64
    assert second["fit"] == first["fit"]  # the fit reads the raw score whatever the reporting temperature
    bound = 1 / (128 * t)
    print(f"fitted T {t!r}: NLL {first['summary']['nll']!r} at T = 1, {first['fit']['nll_fitted']!r} from the "
          f"histogram at the fitted T, {second['summary']['nll']!r} exact in the second run; bound {bound:.3e}")
    assert abs(second["summary"]["nll"] - first["fit"]["nll_fitted"]) <= bound
    assert second["summary"]["nll"] <= first["summary"]["nll"] + bound
    assert second["summary"]["pixels"] == first["summary"]["pixels"]


def test_eval_cli_calibration_leaves_the_rest_alone(cli):
    a = open(cli["on_dir"] / "performance.json", "rb").read()
    b = open(cli["off_dir"] / "performance.json", "rb").read()
    assert a == b
    assert sorted(os.listdir(cli["off_dir"])) == ["performance.json"]
    assert sorted(os.listdir(cli["on_dir"])) == ["calibration.json", "calibration_bins.csv", "performance.json"]
