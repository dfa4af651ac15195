"""The one-pass risk-coverage sweep on the GPU: `selunet_seg_metrics_sweep` against numpy and against
`selunet_seg_metrics` (integer counts: bit-exact), `metrics.SelectiveSweep`, and the eval CLI's
--s_cut_off_sweep / --target_coverage against one plain eval run per cut-off and the CPU oracle.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import unet_b_cpu as O
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import eval as EV
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT
from selectivenet_for_semantic_segmentation_binary_amd.data import load_test_set_for_tests
from selectivenet_for_semantic_segmentation_binary_amd.synthetic import preprocess

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_OUT = np.float32(MT.logit_threshold("eval", 0.5))
F32 = np.float32


# ----------------------------------------------------------------------------- kernel level
def run_sweep(out, sel, tgt, thr, calls=1, t_out=T_OUT):
    """bins [(k+1), 5] of `calls` accumulating kernel calls on host arrays (or device tensors)."""
    dev = [a if torch.is_tensor(a) else torch.tensor(a, device=DEV) for a in (out, sel, tgt)]
    tt = torch.tensor(np.asarray(thr, F32), device=DEV)
    bins = torch.zeros(len(thr) + 1, 5, dtype=torch.int64, device=DEV)
    for _ in range(calls):
        K.call("selunet_seg_metrics_sweep", K.ptr(dev[0]), K.ptr(dev[1]), K.ptr(dev[2]), dev[0].numel(), float(t_out),
               K.ptr(tt), len(thr), K.ptr(bins), K.stream_ptr())
    return bins.cpu().numpy()


def suffix(bins):
    """row j: the sum of the bins above j = the counts at threshold j."""
    return np.cumsum(bins[::-1], axis=0)[::-1][1:]


def numpy_rows(out, sel, tgt, thr, t_out=T_OUT):
    """Per threshold [cm00, cm01, cm10, cm11, selected] from the Evaluator's own matrix code."""
    lab = tgt.astype("uint8")
    pred = (out >= t_out).astype("uint8")
    rows = []
    with np.errstate(invalid="ignore"):
        for t in thr:
            smask = sel >= F32(t)
            cm = O.confusion_matrix(lab, pred, selection=smask)  # labels >= 2 are left out there
            rows.append(list(cm.reshape(-1).astype(np.int64)) + [int(smask.sum())])
    return np.array(rows, np.int64)


def numpy_bins(out, sel, tgt, thr, t_out=T_OUT):
    """The bins themselves: bin = #{j: sel >= thr[j]} (NaN -> 0), class = cm cell or label >= 2."""
    thr = np.asarray(thr, F32)
    b = np.searchsorted(thr, sel, side="right")
    b[np.isnan(sel)] = 0
    lab = tgt.astype("uint8").astype(np.int64)
    cls = np.where(lab < 2, lab * 2 + (out >= t_out), 4)
    h = np.bincount(b * 5 + cls, minlength=(len(thr) + 1) * 5).reshape(len(thr) + 1, 5)
    h[:, 4] = h.sum(1)
    return h.astype(np.int64)


def edge_case(thr, seed):
    """As test_seg_metrics_bit_exact: logits ~ N(0, 1e-6) and a ragged tail, with every threshold, its
    two fp32 neighbours, +-0, +-inf, nan and saturated values in both `out` and `sel`; a few labels
    >= 2 (counted in `pixels` only). p = 4*3*50 + 3, or the next 4*3*50*m + 3 that holds the edge
    values twice (k = 256 has 3 * 257 + 7 of them)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.concatenate([np.asarray(thr, F32), [T_OUT]]).astype(F32)
    with np.errstate(invalid="ignore"):
        edge = np.concatenate([t, np.nextafter(t, F32(-np.inf)), np.nextafter(t, F32(np.inf)),
                               np.array([0, -0.0, np.inf, -np.inf, np.nan, 40, -40], F32)]).astype(F32)
    m = 1
    while 4 * 3 * 50 * m + 3 < 2 * len(edge) + 5:
        m += 1
    p = 4 * 3 * 50 * m + 3
    out = rng.normal(0, 1e-6, p).astype(F32)
    sel = rng.normal(0, 1e-6, p).astype(F32)
    out[:len(edge)] = edge
    sel[5:5 + len(edge)] = edge
    sel[-len(edge):] = edge[::-1]  # the ragged tail sees edge values too
    tgt = (rng.random(p) > 0.4).astype(F32)
    tgt[rng.choice(p, 9, replace=False)] = np.array([2, 255, 2, 255, 2, 255, 2, 255, 2], F32)
    return out, sel, tgt


T05 = F32(MT.logit_threshold("eval", 0.5))
THRESHOLDS = {
    "k1": np.array([T05], F32),
    "k6": np.array([-np.inf, -5e-7, T05, T05, 7e-7, np.inf], F32),  # a duplicate pair, infinite ends
    "k256": np.linspace(-3e-6, 3e-6, 256).astype(F32),
}


@pytest.mark.parametrize("name", list(THRESHOLDS))
def test_sweep_kernel_bit_exact_against_numpy(name):
    thr = THRESHOLDS[name]
    assert np.all(thr[1:] >= thr[:-1])
    out, sel, tgt = edge_case(thr, seed=11)
    p = out.size
    assert p % 4 == 3 and (p == 603 or name == "k256")
    want = numpy_rows(out, sel, tgt, thr)
    assert want[:, :4].sum() > 0 and len(set(want[:, 4])) >= min(len(thr), 3)  # the case is not degenerate
    for calls in (1, 2):  # the kernel accumulates
        bins = run_sweep(out, sel, tgt, thr, calls)
        assert bins.shape == (len(thr) + 1, 5) and (bins >= 0).all()
        assert np.array_equal(suffix(bins), calls * want), name
        assert bins[:, 4].sum() == calls * p
        assert np.array_equal(bins, calls * numpy_bins(out, sel, tgt, thr)), name


def test_sweep_kernel_equals_seg_metrics_per_threshold():
    thr = THRESHOLDS["k6"]
    out, sel, tgt = edge_case(thr, seed=12)
    ot, st, tt = (torch.tensor(a, device=DEV) for a in (out, sel, tgt))
    bins = run_sweep(ot, st, tt, thr)
    rows = suffix(bins)
    for j, t in enumerate(thr):
        counts = torch.zeros(6, dtype=torch.int64, device=DEV)
        K.call("selunet_seg_metrics", K.ptr(ot), K.ptr(st), K.ptr(tt), ot.numel(), float(T_OUT), float(t),
               K.ptr(counts), K.stream_ptr())
        c = counts.cpu().numpy()
        assert np.array_equal(rows[j], c[:5]), (j, rows[j], c)
        assert bins[:, 4].sum() == c[5]


# 16 x 256 x 256 + 3 pixels: the kernel's grid is capped at 256 workgroups of 256 threads x 4 pixels, so
# every workgroup makes four stride passes (a single pass would need a cap of 1024 or more), plus the tail
P_BIG = 16 * 256 * 256 + 3
THR_BIG = np.linspace(-4, 4, 101).astype(F32)  # 0.0 is threshold 50


@pytest.fixture(scope="module")
def big():
    rng = np.random.Generator(np.random.PCG64(13))
    out = rng.normal(0, 1, P_BIG).astype(F32)
    tgt = (rng.random(P_BIG) > 0.4).astype(F32)
    tgt[rng.choice(P_BIG, 1000, replace=False)] = 2.0
    return {"out": out, "tgt": tgt, "out_d": torch.tensor(out, device=DEV), "tgt_d": torch.tensor(tgt, device=DEV)}


def test_sweep_kernel_many_workgroups_uniform_bins(big):
    rng = np.random.Generator(np.random.PCG64(14))
    sel = rng.uniform(-4.08, 4.08, P_BIG).astype(F32)  # 102 bins of width 0.08
    want = numpy_bins(big["out"], sel, big["tgt"], THR_BIG)
    assert (want[:, 4] > P_BIG // 102 // 2).all()
    bins = run_sweep(big["out_d"], torch.tensor(sel, device=DEV), big["tgt_d"], THR_BIG)
    assert np.array_equal(bins, want)
    js = [0, 37, 50, 100]
    assert np.array_equal(suffix(bins)[js], numpy_rows(big["out"], sel, big["tgt"], THR_BIG[js]))
    assert bins[:, 4].sum() == P_BIG


@pytest.mark.parametrize("value,bin_", [(0.0, 51), (-np.inf, 0), (np.inf, 101)])
def test_sweep_kernel_every_pixel_in_one_bin(big, value, bin_):
    """Maximum contention on one bin's counters: narrow or overflowing counters and lost on-chip
    updates show here."""
    sel = np.full(P_BIG, value, F32)
    want = numpy_bins(big["out"], sel, big["tgt"], THR_BIG)
    assert want[bin_, 4] == P_BIG and np.count_nonzero(want[:, 4]) == 1 and (want[bin_] > 0).all()
    bins = run_sweep(big["out_d"], torch.tensor(sel, device=DEV), big["tgt_d"], THR_BIG)
    assert np.array_equal(bins, want)
    js = [0, 50, 100]
    assert np.array_equal(suffix(bins)[js], numpy_rows(big["out"], sel, big["tgt"], THR_BIG[js]))


# ----------------------------------------------------------------------------- SelectiveSweep
def test_selective_sweep_class():
    sw = MT.SelectiveSweep(DEV, [0.9, 0.1, 0.5, 0.1, 0.9, 0.3])
    assert sw.s_cut_offs == [0.1, 0.3, 0.5, 0.9]
    assert sw.thresholds.device.type == "cuda" and sw.thresholds.dtype == torch.float32
    assert sw.thresholds.cpu().tolist() == [MT.logit_threshold("eval", c) for c in sw.s_cut_offs]
    assert tuple(sw.bins.shape) == (5, 5) and sw.bins.dtype == torch.int64 and sw.bins.device.type == "cuda"
    rng = np.random.Generator(np.random.PCG64(15))
    out, sel = (rng.normal(0, 2, (2, 5, 7)).astype(F32) for _ in range(2))
    tgt = (rng.random((2, 5, 7)) > 0.5).astype(F32)
    ot, st, tt = (torch.tensor(a, device=DEV) for a in (out, sel, tgt))
    sw.add_batch(ot, tt, st)
    raw = sw.raw()
    assert raw.shape == (5, 5) and raw.dtype == np.int64 and raw[:, 4].sum() == 70
    assert np.array_equal(raw, numpy_bins(out.ravel(), sel.ravel(), tgt.ravel(), sw.thresholds.cpu().numpy()))
    rows = sw.curve()
    for r in rows:  # each row is what SegMetrics counts at that cut-off alone
        m = MT.SegMetrics(DEV, selective=True, rule="eval", s_cut_off=r["s_cut_off"])
        m.add_batch(ot, tt, st)
        assert np.array_equal(np.array(r["confusion_matrix"]), m.confusion_matrix())
        assert (r["selected"], r["total"]) == m.selected_total()
    sw.reset()
    assert not sw.raw().any()
    for bad in ((ot.transpose(1, 2), tt, st), (ot, tt, st.transpose(1, 2)), (ot.double(), tt, st),
                (ot, tt.to(torch.int64), st), (ot.cpu(), tt, st)):
        with pytest.raises(RuntimeError):
            sw.add_batch(*bad)
    for bad in ((ot[:1].contiguous(), tt, st), (ot, tt, st[:1].contiguous()), (ot, tt, None)):
        with pytest.raises(ValueError):
            sw.add_batch(*bad)
    assert not sw.raw().any()
    with pytest.raises(ValueError):
        MT.SelectiveSweep(DEV, np.linspace(0.2, 0.8, 257))


# ----------------------------------------------------------------------------- eval CLI
QUANTILES = (0.1, 0.25, 0.5, 0.75, 0.9)


def calibrated_checkpoint(path):
    """A checkpoint whose eval-mode heads spread: the seed-0 state with the selection and prediction
    heads' weights x 64 and each head's bias moved by the median of its oracle eval-mode output (a
    fresh network's selection logits span < 0.1 and its predictions are one class). Returns the
    oracle's eval-mode output and selection logits and the labels of the test set."""
    params, buffers = O.make_state(0, "RGB", True)
    imgs, labs = load_test_set_for_tests("synthetic:8", 64, 2)
    x, lab = preprocess(imgs, labs)
    with torch.no_grad():
        params["conv_select.weight"].mul_(64)
        params["conv1x1.weight"].mul_(64)
        o, s, _ = O.forward(params, buffers, torch.tensor(x), True, training=False)
        params["conv1x1.bias"].sub_(o.median())
        params["conv_select.bias"].sub_(s.median())
        o, s, _ = O.forward(params, buffers, torch.tensor(x), True, training=False)
    sd = {k: v.detach().clone() for k, v in params.items()}
    sd.update({k: v.clone() for k, v in buffers.items()})
    torch.save({"net": sd}, path)
    return o.numpy(), s.numpy(), lab


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sweep_cli")
    ck = tmp / "checkpoint"
    ck.mkdir()
    o, s, lab = calibrated_checkpoint(ck / "model_epoch1.pth")
    q = np.quantile(s.astype(np.float64), QUANTILES)
    cuts = sorted([0.0, 1.0] + [float(1 / (1 + np.exp(-v))) for v in q])
    base = ["--data_dir", "synthetic:8", "--patch_size", "64", "--test_fold", "2", "--model_dir", str(ck),
            "--model_arch", "UNet_B", "--selective", "1", "--select_eval", "1", "--batch_size", "4"]

    def run(name, *extra):
        out = tmp / name
        res = EV.evaluate(EV.parse_arguments(base + ["--save_dir", str(out)] + list(extra)))
        return res, out

    swept, sweep_dir = run("sweep", "--s_cut_off_sweep", *[repr(c) for c in reversed(cuts)], "--target_coverage", "0.5")
    plain = {c: run(f"plain{i}", "--s_cut_off", repr(c))[0] for i, c in enumerate(cuts)}
    _, default_dir = run("default")
    return {"o": o, "s": s, "lab": lab, "cuts": cuts, "swept": swept, "sweep_dir": sweep_dir, "plain": plain,
            "default_dir": default_dir}


def oracle_row(c, cut):
    pred = O.eval_pred_mask(c["o"])
    sel = O.eval_pred_mask(c["s"], cut_off=cut)
    return O.confusion_matrix(c["lab"].astype("uint8"), pred, selection=sel), int(sel.sum())


def test_eval_cli_sweep_oracle_preconditions(cli):
    """On the oracle alone, so the comparisons below cannot pass vacuously."""
    rows = [oracle_row(cli, c) for c in cli["cuts"]]
    cov = {sel / cli["lab"].size for _, sel in rows}
    assert len([v for v in cov if 0 < v < 1]) >= 5, sorted(cov)
    assert set(np.unique(cli["lab"].astype("uint8"))) == {0, 1}
    assert set(np.unique(O.eval_pred_mask(cli["o"]))) == {0, 1}
    for (cm, _), c in zip(rows, cli["cuts"]):
        if 0 < c < 1:
            assert (cm > 0).all(), (c, cm)


def test_eval_cli_sweep_rows_equal_plain_runs(cli):
    doc = json.load(open(cli["sweep_dir"] / "risk_coverage.json"))
    curve = doc["curve"]
    assert [r["s_cut_off"] for r in curve] == cli["cuts"]
    assert [r["s_cut_off"] for r in cli["swept"]["risk_coverage"]["curve"]] == cli["cuts"]
    for r in curve:
        p = cli["plain"][r["s_cut_off"]]
        assert r["confusion_matrix"] == p["confusion_matrix"], r["s_cut_off"]
        total = r["total"]
        assert total == cli["lab"].size
        assert (total - r["selected"]) / total == p["rejection_ratio"], r["s_cut_off"]
        if r["selected"]:
            assert (r["Acc"], r["mIoU"], r["Prec"], r["Recall"], r["F1_Score"], r["IoU_class"]) == \
                (p["Acc"], p["mIoU"], p["Prec"], p["Recall"], p["F1_Score"], p["IoU_class"]), r["s_cut_off"]
            assert r["risk"] == 1 - p["Acc"]


def test_eval_cli_sweep_rows_match_oracle(cli):
    """<= 1e-3 of the pixels may differ per row: those whose logit lies within fp32 rounding of a cut
    (the cap of test_gpu_train.test_eval_cli_matches_oracle_metrics)."""
    curve = json.load(open(cli["sweep_dir"] / "risk_coverage.json"))["curve"]
    n = cli["lab"].size
    for r in curve:
        cm, sel = oracle_row(cli, r["s_cut_off"])
        d = np.abs(np.array(r["confusion_matrix"]) - cm).sum()
        print(f"cut-off {r['s_cut_off']:.6f}: {int(d)} of {n} matrix counts, {abs(r['selected'] - sel)} selected "
              "pixels differ from the oracle")
        assert d <= 1e-3 * n, (r["s_cut_off"], r["confusion_matrix"], cm)
        assert abs(r["selected"] - sel) <= 1e-3 * n, (r["s_cut_off"], r["selected"], sel)


def test_eval_cli_sweep_calibration_and_files(cli):
    doc = json.load(open(cli["sweep_dir"] / "risk_coverage.json"))
    curve = doc["curve"]
    cov = [r["coverage"] for r in curve]
    assert all(a >= b for a, b in zip(cov, cov[1:])), cov  # non-increasing down the table
    want = max(c for c, v in zip(cli["cuts"], cov) if v >= 0.5)
    assert doc["target_coverage"] == 0.5 and doc["calibrated_s_cut_off"] == want
    assert doc["calibrated"]["s_cut_off"] == want and doc["calibrated"]["coverage"] >= 0.5
    assert doc["calibrated"] == next(r for r in curve if r["s_cut_off"] == want)
    assert 0 < want < 1
    last = curve[-1]  # cut-off 1.0: nothing selected, NaN metrics, and the run went through
    assert last["s_cut_off"] == 1.0 and last["selected"] == 0 and last["coverage"] == 0.0
    assert math.isnan(last["Acc"]) and math.isnan(last["risk"]) and math.isnan(last["mIoU"])
    assert curve[0]["s_cut_off"] == 0.0 and curve[0]["coverage"] == 1.0
    lines = open(cli["sweep_dir"] / "risk_coverage.csv").read().strip().split("\n")
    assert lines[0].startswith("s_cut_off,coverage,") and len(lines) == 1 + len(curve)
    assert [float(ln.split(",")[0]) for ln in lines[1:]] == cli["cuts"]
    # performance.json is what the same command writes without the sweep flags
    a = open(cli["sweep_dir"] / "performance.json", "rb").read()
    b = open(cli["default_dir"] / "performance.json", "rb").read()
    assert a == b
    assert not os.path.exists(cli["default_dir"] / "risk_coverage.json")


def test_eval_cli_sweep_unreachable_coverage_and_refusals(cli, tmp_path):
    ck = [str(p) for p in cli["sweep_dir"].parent.glob("checkpoint")][0]
    base = ["--data_dir", "synthetic:8", "--patch_size", "64", "--test_fold", "2", "--model_dir", ck, "--batch_size", "4",
            "--save_dir", str(tmp_path)]
    res = EV.evaluate(EV.parse_arguments(base + ["--selective", "1", "--s_cut_off_sweep", "0.5", "1.0",
                                                 "--target_coverage", "0.99"]))
    doc = json.load(open(tmp_path / "risk_coverage.json"))
    assert doc["calibrated_s_cut_off"] is None and doc["calibrated"] is None and "unreachable" in doc["calibration_note"]
    assert res["risk_coverage"]["calibrated_s_cut_off"] is None
    with pytest.raises(ValueError):  # a sweep needs the selection head
        EV.evaluate(EV.parse_arguments(base + ["--s_cut_off_steps", "4"]))
