"""The per-patch report on the GPU: `selunet_seg_metrics_rows` and `selunet_patch_auc` against numpy
(integers: bit-exact), against `selunet_seg_metrics` and against the reference's `get_performance`
fixture, `metrics.PatchReport`, and the eval CLI's --patch_report.
"""
import json
import math

import numpy as np
import pytest
import torch

import selectivenet_for_semantic_segmentation_binary_amd as S
from oracle import unet_b_cpu as O
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import data as D
from selectivenet_for_semantic_segmentation_binary_amd import eval as EV
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT
from selectivenet_for_semantic_segmentation_binary_amd import net_utils
from selectivenet_for_semantic_segmentation_binary_amd.synthetic import preprocess
from tests._patch_ref import auc_bound, fixture_cases, numpy_auc, numpy_counts, same

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
T_OUT = F32(MT.logit_threshold("eval", 0.5))
T_SEL = F32(0.1)
CHUNK = K.AUC_CHUNK
EDGE = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-42, -1e-42, 1e-45, -1e-45, 3e38, -3e38], F32)


# ----------------------------------------------------------------------------- kernel level
def run_rows(out, sel, tgt, calls=1, t_out=T_OUT, t_sel=T_SEL):
    """(counts [n][6], auc [n][4]) of `calls` accumulating calls of each kernel on [n][hw] arrays."""
    n, hw = out.shape
    ot, tt = (a if torch.is_tensor(a) else torch.tensor(a, device=DEV) for a in (out, tgt))
    st = None if sel is None else (sel if torch.is_tensor(sel) else torch.tensor(sel, device=DEV))
    counts = torch.zeros(n, 6, dtype=torch.int64, device=DEV)
    auc = torch.zeros(n, 4, dtype=torch.int64, device=DEV)
    for _ in range(calls):
        K.call("selunet_seg_metrics_rows", K.ptr(ot), K.ptr(st), K.ptr(tt), n, hw, float(t_out), float(t_sel),
               K.ptr(counts), K.stream_ptr())
        K.call("selunet_patch_auc", K.ptr(ot), K.ptr(st), K.ptr(tt), n, hw, float(t_sel), K.ptr(auc), K.stream_ptr())
    return counts.cpu().numpy(), auc.cpu().numpy()


def numpy_rows(out, sel, tgt, t_out=T_OUT, t_sel=T_SEL):
    counts = [numpy_counts(out[i], None if sel is None else sel[i], tgt[i], t_out, t_sel) for i in range(len(out))]
    auc = [numpy_auc(out[i], None if sel is None else sel[i], tgt[i], t_sel) for i in range(len(out))]
    return np.array(counts, np.int64), np.array(auc, np.int64)


def sprinkle(rng, out, tgt, times=3):
    """The edge logits on both labels at random places, and in the image's last four pixels (the ragged
    last chunk, which may hold only them)."""
    at = rng.choice(out.size - 4, times * 2 * len(EDGE), replace=False)
    out[at] = np.tile(EDGE, times * 2)
    tgt[at] = np.repeat(np.array([0, 1] * times, F32), len(EDGE))
    out[-4:] = np.array([-0.0, np.inf, 1e-42, np.nan], F32)
    tgt[-4:] = np.array([0, 1, 0, 0], F32)


def make_case(hw, variant, seed):
    """Three images that differ. 'mixed': (0) normal logits with the edge values and labels >= 2, (1)
    logits quantised to 0.5 with 5 % positives, (2) all logits equal. 'degenerate': (0) all positive,
    (1) all negative, (2) both classes and the edge values, its every pixel rejected by the selection.
    The selection logits hold NaNs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = rng.normal(0, 1, (3, hw)).astype(F32)
    tgt = (rng.random((3, hw)) > 0.5).astype(F32)
    sel = rng.normal(0.1, 1, (3, hw)).astype(F32)
    sel[:, rng.choice(hw, 7, replace=False)] = np.nan
    sel[:, rng.choice(hw, 7, replace=False)] = T_SEL  # on the threshold: selected
    if variant == "mixed":
        sprinkle(rng, out[0], tgt[0])
        tgt[0, rng.choice(hw - 4, 9, replace=False)] = np.array([2, 255, 2, 255, 2, 255, 2, 255, 2], F32)
        out[1] = np.round(out[1] * 2) / 2
        tgt[1] = (rng.random(hw) < 0.05).astype(F32)
        tgt[1, :2] = (0, 1)
        out[2] = F32(0.25)
    else:
        tgt[0], tgt[1] = 1.0, 0.0
        out[1, :11] = EDGE
        sprinkle(rng, out[2], tgt[2])
        sel[2] = np.where(rng.random(hw) < 0.5, F32(-3), np.nextafter(T_SEL, F32(-np.inf)))
        sel[2, 5] = np.nan
    return out, sel, tgt


HWS = (576, CHUNK, CHUNK + 1088, 2 * CHUNK + 4)  # under one chunk, one chunk, a ragged second, a third of 4 pixels


@pytest.mark.parametrize("variant", ["mixed", "degenerate"])
@pytest.mark.parametrize("hw", HWS)
def test_kernels_bit_exact_against_numpy(hw, variant):
    out, sel, tgt = make_case(hw, variant, seed=hw + len(variant))
    assert out.shape == (3, hw) and hw % 4 == 0
    for s in (None, sel):
        want_c, want_a = numpy_rows(out, s, tgt)
        # the case is what it claims to be
        if variant == "mixed":
            assert want_a[0, 3] > 0 and want_c[0, :4].sum() < (hw if s is None else want_c[0, 4])  # NaNs, labels >= 2
            assert (want_a[:, 1:3] > 0).all()
            assert want_a[2, 0] == want_a[2, 1] * want_a[2, 2]  # all equal: every pair a tie
        else:
            assert want_a[0, 2] == 0 and want_a[1, 1] == 0 and not want_a[:2, 0].any()
            if s is None:
                assert want_a[2, 0] > 0 and want_a[2, 3] > 0
            else:
                assert not want_a[2].any() and not want_c[2, :5].any() and want_c[2, 5] == hw
        if s is not None:
            assert (want_c[:2, 4] > 0).all() and (want_c[:2, 4] < hw).all()
        for calls in (1, 2):  # the kernels accumulate
            got_c, got_a = run_rows(out, s, tgt, calls)
            assert np.array_equal(got_c, calls * want_c), (hw, variant, s is None, calls, got_c, want_c)
            assert np.array_equal(got_a, calls * want_a), (hw, variant, s is None, calls, got_a, want_a)


def test_kernels_on_a_megapixel_image():
    """hw = 2^20, the largest the calls take: 256 chunks, and the 32-bit partial counts at their
    largest — every positive above every negative, so each positive adds two full chunks per workgroup."""
    hw = 1 << 20
    rng = np.random.Generator(np.random.PCG64(21))
    tgt = (rng.random((1, hw)) > 0.5).astype(F32)
    out = (rng.random((1, hw)).astype(F32) + 1) * np.where(tgt == 1, F32(1), F32(-1))
    sel = rng.normal(0.1, 1, (1, hw)).astype(F32)
    for s in (None, sel):
        want_c, want_a = numpy_rows(out, s, tgt)
        assert want_a[0, 0] == 2 * want_a[0, 1] * want_a[0, 2] and (s is not None or want_a[0, 0] > 1 << 38)
        got_c, got_a = run_rows(out, s, tgt)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_a, want_a), (got_c, want_c, got_a, want_a)


def test_kernels_on_more_images_than_one_launch_row():
    """n = 32768 + 5 images of four pixels: the calls split the images over two launches."""
    n, hw = 32768 + 5, 4
    rng = np.random.Generator(np.random.PCG64(22))
    out = np.round(rng.normal(0, 1, (n, hw)) * 2).astype(F32) / 2
    tgt = (rng.random((n, hw)) > 0.5).astype(F32)
    sel = rng.normal(0.1, 1, (n, hw)).astype(F32)
    for s in (None, sel):
        smask = np.ones((n, hw), bool) if s is None else s >= T_SEL
        pos, neg = smask & (tgt == 1), smask & (tgt == 0)
        pair = pos[:, :, None] & neg[:, None, :]
        lt, eq = out[:, None, :] < out[:, :, None], out[:, None, :] == out[:, :, None]
        want_a = np.stack([((2 * lt + eq) * pair).sum((1, 2)), pos.sum(1), neg.sum(1), np.zeros(n, np.int64)], 1)
        pred = out >= T_OUT
        want_c = np.stack([(neg & ~pred).sum(1), (neg & pred).sum(1), (pos & ~pred).sum(1), (pos & pred).sum(1),
                           smask.sum(1), np.full(n, hw)], 1)
        got_c, got_a = run_rows(out, s, tgt)
        assert np.array_equal(got_a[-6:], want_a[-6:]) and np.array_equal(got_a, want_a)
        assert np.array_equal(got_c[-6:], want_c[-6:]) and np.array_equal(got_c, want_c)
    # spot-check the vectorised restatement against the per-image one
    i = n - 3
    assert numpy_auc(out[i], sel[i], tgt[i], T_SEL) == list(want_a[i])
    assert numpy_counts(out[i], sel[i], tgt[i], T_OUT, T_SEL) == list(want_c[i])


# ----------------------------------------------------------------------------- consistency
def test_rows_sum_to_seg_metrics_of_the_batch():
    out, sel, tgt = make_case(CHUNK + 1088, "mixed", seed=31)
    ot, st, tt = (torch.tensor(a, device=DEV) for a in (out, sel, tgt))
    for s in (None, st):
        got_c, got_a = run_rows(ot, s, tt)
        counts = torch.zeros(6, dtype=torch.int64, device=DEV)
        K.call("selunet_seg_metrics", K.ptr(ot), K.ptr(s), K.ptr(tt), ot.numel(), float(T_OUT), float(T_SEL),
               K.ptr(counts), K.stream_ptr())
        assert np.array_equal(got_c.sum(0), counts.cpu().numpy())
        # every counted pixel is a positive, a negative or a NaN logit
        assert np.array_equal(got_a[:, 1:].sum(1), got_c[:, :4].sum(1))


def test_gpu_auc_within_the_bound_of_the_reference():
    cases, t_out = fixture_cases()
    finite = 0
    for name, lab, logit, _, want in cases:
        hw = lab.size
        c, a = run_rows(logit[None], None, lab.astype(F32)[None], t_out=t_out)
        assert list(a[0]) == numpy_auc(logit, None, lab.astype(F32), 0.0), name
        got = MT.patch_performance(c[0, :4].reshape(2, 2), *a[0, :3])
        for k, w in zip(("accuracy", "recall", "precision", "f1_score"), want[:4]):
            assert same(got[k], w), (name, k, got[k], w)
        if math.isnan(want[4]):
            assert math.isnan(got["auc_score"]), name
            continue
        finite += 1
        err = abs(got["auc_score"] - want[4])
        print(f"{name}: |GPU two_u / (2 n_pos n_neg) - reference AUC| = {err:.3g} (bound {auc_bound(hw):.3g})")
        assert err <= auc_bound(hw), (name, got["auc_score"], want[4])
    assert finite >= 10


def test_two_runs_give_the_same_integers():
    rng = np.random.Generator(np.random.PCG64(33))
    out = torch.tensor(rng.normal(0, 1, (4, 128 * 128)).astype(F32), device=DEV)
    sel = torch.tensor(rng.normal(0, 1, (4, 128 * 128)).astype(F32), device=DEV)
    tgt = torch.tensor((rng.random((4, 128 * 128)) > 0.3).astype(F32), device=DEV)
    first = run_rows(out, sel, tgt)
    second = run_rows(out, sel, tgt)
    assert first[1][:, 0].min() > 0
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


# ----------------------------------------------------------------------------- PatchReport
def test_patch_report_class():
    rng = np.random.Generator(np.random.PCG64(34))
    batches = []
    for n in (3, 2):  # a smaller last batch
        out, sel = (rng.normal(0, 2, (n, 12, 20)).astype(F32) for _ in range(2))
        tgt = (rng.random((n, 12, 20)) > 0.5).astype(F32)
        batches.append((out, sel, tgt))
    batches[1][2][1] = 0.0  # the last patch has one class
    t_sel = MT.logit_threshold("eval", 0.3)
    for selective in (False, True):
        rep = MT.PatchReport(DEV, selective=selective, s_cut_off=0.3)
        dev = [[torch.tensor(a, device=DEV) for a in b] for b in batches]
        rep.add_batch(dev[0][0], dev[0][2], dev[0][1], ids=["a_0_0", "a_0_256", "b_256_0"])
        rep.add_batch(dev[1][0], dev[1][2], dev[1][1] if selective else None)
        rows = rep.rows()
        assert [r["index"] for r in rows] == list(range(5))
        assert [r["id"] for r in rows] == ["a_0_0", "a_0_256", "b_256_0", "patch_3", "patch_4"]
        flat = [(o[i].ravel(), s[i].ravel(), t[i].ravel()) for o, s, t in batches for i in range(len(o))]
        for r, (o, s, t) in zip(rows, flat):
            c, a = numpy_counts(o, None, t, T_OUT, t_sel), numpy_auc(o, None, t, t_sel)
            assert [r[k] for k in ("cm00", "cm01", "cm10", "cm11")] == c[:4] and r["pixels"] == 240
            assert [r[k] for k in ("two_u", "n_pos", "n_neg", "n_nan")] == a
            perf = MT.patch_performance([c[:2], c[2:4]], *a[:3])
            assert all(same(r[k], v) for k, v in perf.items())
            assert ("selected" in r) == selective and ("sel_auc_score" in r) == selective
            if selective:
                c, a = numpy_counts(o, s, t, T_OUT, t_sel), numpy_auc(o, s, t, t_sel)
                assert [r["sel_" + k] for k in ("cm00", "cm01", "cm10", "cm11")] == c[:4]
                assert [r["sel_" + k] for k in ("two_u", "n_pos", "n_neg", "n_nan")] == a
                assert r["selected"] == c[4] and 0 < c[4] < 240 and r["coverage"] == c[4] / 240
                perf = MT.patch_performance([c[:2], c[2:4]], *a[:3])
                assert all(same(r["sel_" + k], v) for k, v in perf.items())
        assert math.isnan(rows[4]["auc_score"]) and not math.isnan(rows[0]["auc_score"])
        ot, st, tt = dev[0]
        for bad in ((ot.transpose(1, 2), tt, st), (ot.double(), tt, st), (ot, tt.to(torch.int64), st), (ot.cpu(), tt, st),
                    (ot, tt, st.transpose(1, 2))):
            with pytest.raises(RuntimeError):
                rep.add_batch(*bad)
        for bad in ((ot[:1].contiguous(), tt, st), (ot.reshape(3, -1), tt.reshape(3, -1), st.reshape(3, -1)),
                    (ot, tt, st[:1].contiguous())):
            with pytest.raises(ValueError):
                rep.add_batch(*bad)
        with pytest.raises(ValueError):
            rep.add_batch(ot, tt, st, ids=["only_one"])
        if selective:
            with pytest.raises(ValueError):
                rep.add_batch(ot, tt, None)
        assert len(rep.rows()) == 5  # a refused batch adds nothing
        rep.reset()
        assert rep.rows() == []


# ----------------------------------------------------------------------------- eval CLI
def calibrated_checkpoint(path):
    """The checkpoint of tests/test_gpu_sweep.py, made the same way: the seed-0 state with the selection
    and prediction heads' weights x 64 and each head's bias moved by the median of its oracle eval-mode
    output, so that eval-mode predictions and selections spread over both sides of their cut-offs."""
    params, buffers = O.make_state(0, "RGB", True)
    imgs, labs = D.load_test_set_for_tests("synthetic:8", 64, 2)
    x, lab = preprocess(imgs, labs)
    with torch.no_grad():
        params["conv_select.weight"].mul_(64)
        params["conv1x1.weight"].mul_(64)
        o, s, _ = O.forward(params, buffers, torch.tensor(x), True, training=False)
        params["conv1x1.bias"].sub_(o.median())
        params["conv_select.bias"].sub_(s.median())
    sd = {k: v.detach().clone() for k, v in params.items()}
    sd.update({k: v.clone() for k, v in buffers.items()})
    torch.save({"net": sd}, path)
    return lab


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("patch_cli")
    ck = tmp / "checkpoint"
    ck.mkdir()
    lab = calibrated_checkpoint(ck / "model_epoch1.pth")
    base = ["--data_dir", "synthetic:8", "--patch_size", "64", "--test_fold", "2", "--model_dir", str(ck),
            "--model_arch", "UNet_B", "--selective", "1", "--batch_size", "4"]

    def run(name, *extra):
        out = tmp / name
        res = EV.evaluate(EV.parse_arguments(base + ["--save_dir", str(out)] + list(extra)))
        return res, out

    # the logits of the same network on the same batches, obtained here
    net = S.UNet_B("RGB", selective=True, compute_dtype=torch.float32)
    net_utils.net_test_load(str(ck / "model_epoch1.pth"), net)
    net = net.to(DEV).train(False)
    ds = D.PatchSet(*D.load_test_set_for_tests("synthetic:8", 64, 2))
    loader = D.BatchLoader(ds, 4, shuffle=False, random_flip=False, device=torch.device(DEV, 0), input_type="RGB")
    logits = []
    with torch.no_grad():
        for x, target in loader:
            o, s, _ = net(x)
            logits += [(o[i].cpu().numpy().ravel(), s[i].cpu().numpy().ravel(), target[i].cpu().numpy().ravel())
                       for i in range(o.shape[0])]
    return {"lab": lab, "logits": logits, "base": base, "tmp": tmp,
            "sel_on": run("sel_on", "--select_eval", "1", "--patch_report", "1"),
            "sel_off": run("sel_off", "--select_eval", "1"),
            "all_on": run("all_on", "--patch_report", "1")}


def read_csv(path):
    lines = open(path).read().strip().split("\n")
    head = lines[0].split(",")
    return head, [dict(zip(head, ln.split(","))) for ln in lines[1:]]


def test_eval_cli_patch_report_preconditions(cli):
    """Asserted first: the labels alone give at least half of the patches both classes, and patch 1 one."""
    lab = cli["lab"].reshape(8, -1)
    both = [(row == 1).any() and (row == 0).any() for row in lab]
    assert sum(both) >= 4 and not both[1]
    rows = cli["all_on"][0]["patch_report"]["rows"]
    finite = [math.isfinite(r["auc_score"]) for r in rows]
    assert sum(finite) >= 4 and finite == both
    assert math.isnan(rows[1]["auc_score"])
    assert len(cli["logits"]) == 8 and all(np.array_equal(t, lab[i]) for i, (_, _, t) in enumerate(cli["logits"]))


def test_eval_cli_patch_report_leaves_the_plain_outputs_alone(cli):
    a = open(cli["sel_on"][1] / "performance.json", "rb").read()
    b = open(cli["sel_off"][1] / "performance.json", "rb").read()
    assert a == b
    assert not (cli["sel_off"][1] / "patch_performance.csv").exists()
    assert not (cli["sel_off"][1] / "patch_performance.json").exists()
    assert "patch_report" not in cli["sel_off"][0]
    on = {k: v for k, v in cli["sel_on"][0].items() if k != "patch_report"}
    assert json.dumps(on) == json.dumps(cli["sel_off"][0])


@pytest.mark.parametrize("run", ["sel_on", "all_on"])
def test_eval_cli_patch_report_rows(cli, run):
    res, out = cli[run]
    selective = run == "sel_on"
    rows = res["patch_report"]["rows"]
    assert len(rows) == 8 and [r["index"] for r in rows] == list(range(8))
    assert [r["id"] for r in rows] == [f"patch_{i}" for i in range(8)]
    assert all(r["pixels"] == 64 * 64 for r in rows)
    # the reported confusion matrix is the sum of the patches' (over the selected pixels with --select_eval)
    p = "sel_" if selective else ""
    cm = [[sum(r[p + "cm00"] for r in rows), sum(r[p + "cm01"] for r in rows)],
          [sum(r[p + "cm10"] for r in rows), sum(r[p + "cm11"] for r in rows)]]
    assert cm == res["confusion_matrix"]
    if selective:
        total = 8 * 64 * 64
        assert (total - sum(r["selected"] for r in rows)) / total == res["rejection_ratio"]
        assert 0 < sum(r["selected"] for r in rows) < total
    else:
        assert "selected" not in rows[0]
    # each row's integers from the logits this test obtained itself
    t_sel = MT.logit_threshold("eval", 0.5)
    for r, (o, s, t) in zip(rows, cli["logits"]):
        assert [r[k] for k in ("cm00", "cm01", "cm10", "cm11")] == numpy_counts(o, None, t, T_OUT, t_sel)[:4]
        assert [r[k] for k in ("two_u", "n_pos", "n_neg", "n_nan")] == numpy_auc(o, None, t, t_sel)
        if selective:
            c = numpy_counts(o, s, t, T_OUT, t_sel)
            assert [r["sel_" + k] for k in ("cm00", "cm01", "cm10", "cm11")] + [r["selected"]] == c[:5]
            assert [r["sel_" + k] for k in ("two_u", "n_pos", "n_neg", "n_nan")] == numpy_auc(o, s, t, t_sel)
    # the files say the same
    head, cells = read_csv(out / "patch_performance.csv")
    assert head == list(MT.patch_report_columns(rows)) and len(cells) == 8
    for r, c in zip(rows, cells):
        for k, v in r.items():
            assert c[k] == (repr(v) if isinstance(v, float) else str(v)), (k, c[k], v)
    doc = json.load(open(out / "patch_performance.json"))
    aucs = [r["auc_score"] for r in rows if math.isfinite(r["auc_score"])]
    assert doc["patches"] == 8 and doc["nan_auc"] == 8 - len(aucs) >= 1
    assert doc["mean_auc"] == float(np.mean(aucs)) and doc["median_auc"] == float(np.median(aucs))
    assert ("sel_mean_auc" in doc) == selective


def test_eval_cli_patch_report_printed_line_and_refusal(cli, capsys):
    base = cli["base"] + ["--save_dir", str(cli["tmp"] / "main")]
    EV.main(base)
    off = capsys.readouterr().out
    assert "patch_report" not in off and "per-patch report" not in off
    EV.main(base + ["--patch_report", "1"])
    on = capsys.readouterr().out
    assert "patch_report=True" in on and "per-patch report: 8 patches" in on
    strip = lambda text: [ln for ln in text.split("\n") if not ln.startswith("args=") and "per-patch" not in ln]  # noqa: E731
    assert strip(on) == strip(off)
    # --select_eval needs the selection head, with the report as without: a plain network's checkpoint
    plain = cli["tmp"] / "plain_checkpoint"
    plain.mkdir()
    params, buffers = O.make_state(0, "RGB", False)
    sd = {k: v.detach().clone() for k, v in params.items()}
    sd.update({k: v.clone() for k, v in buffers.items()})
    torch.save({"net": sd}, plain / "model_epoch1.pth")
    args = ["--data_dir", "synthetic:8", "--patch_size", "64", "--test_fold", "2", "--model_dir", str(plain),
            "--batch_size", "4", "--save_dir", str(cli["tmp"] / "plain"), "--patch_report", "1"]
    with pytest.raises(ValueError):
        EV.evaluate(EV.parse_arguments(args + ["--select_eval", "1"]))
    rows = EV.evaluate(EV.parse_arguments(args))["patch_report"]["rows"]  # and works without a selection head
    assert len(rows) == 8 and "selected" not in rows[0] and sum(r["pixels"] for r in rows) == 8 * 64 * 64
