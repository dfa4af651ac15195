"""fp32 eval-mode forwards on the split-fp16 kernels (`fp32_eval_path="split"`).

The bounds are the project's fp32 eval bounds (tests/test_gpu_model.py::test_eval_forward_and_metrics): logits to
1e-4 of the largest |reference logit|, mask bits equal except where the reference logit lies within the measured
logit error of the cut-off, the confusion matrix equal outside those pixels, |dmIoU| < 0.002. What the tests look at:
the fixture, that the split entry points are really the ones called (and nothing changes for training or the default
path), small shapes against the CPU oracle (the split conv at one or two levels only, ragged 16x16 tiles, the CE
heads), an input whose activations exceed the training-mode range bound, the launch-plan cache across the two paths,
the SELUNET_X2=0 fallback in a child process, and the two CLIs.
"""
import contextlib
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import selectivenet_for_semantic_segmentation_binary_amd as S
import selectivenet_for_semantic_segmentation_binary_amd.layout as L
from oracle import unet_b_cpu as O
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import data as D
from selectivenet_for_semantic_segmentation_binary_amd import eval as EV
from selectivenet_for_semantic_segmentation_binary_amd import net_utils
from selectivenet_for_semantic_segmentation_binary_amd import train as TR
from selectivenet_for_semantic_segmentation_binary_amd.engine import fp32_eval_conv_path
from selectivenet_for_semantic_segmentation_binary_amd.synthetic import make_batch
from tests import _golden as G
from tests.test_gpu_patch_report import calibrated_checkpoint

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_ENTRIES = ("selunet_conv3x3_x2", "selunet_gemm_gather_x2", "selunet_act_amax", "selunet_act_bound")
N_CBR = len(L.CBR_LAYERS)


@contextlib.contextmanager
def recorded_calls():
    """The entry-point names `_lib.call` issues inside the block (a recording forward: replays do not pass here)."""
    names, orig = [], K.call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)
    K.call = call
    try:
        yield names
    finally:
        K.call = orig


def gpu_net(params, buffers, selective, path="exact", n_cls=None, dtype=torch.float32):
    """A module holding the oracle state (params, buffers: name -> tensor)."""
    kw = dict(selective=selective, compute_dtype=dtype, fp32_eval_path=path)
    net = S.UNet_B("RGB", **kw) if n_cls is None else S.UNet("RGB", n_cls, **kw)
    with torch.no_grad():
        for k, t in net.named_parameters():
            t.copy_(params[k].detach())
        for k, t in net.named_buffers():
            t.copy_(buffers[k])
    return net.to(DEV).eval()


def heads(o):
    return [t.detach().cpu().numpy() for t in (o if isinstance(o, tuple) else (o,))]


def gpu_eval(net, x):
    with torch.no_grad():
        return heads(net(torch.tensor(x, device=DEV)))


def crop_batch(n, h, w, seed):
    x, lab = make_batch(n, max(h, w), seed=seed)
    return np.ascontiguousarray(x[:, :, :h, :w]), np.ascontiguousarray(lab[:, :h, :w])


@functools.lru_cache(maxsize=None)
def oracle_case(n, h, w, selective, n_cls=None, gain=1.0):
    """The seed-0 state with running statistics from three oracle training-mode forwards (on a batch of another
    seed), and the oracle's eval-mode forward of x * gain in fp32 and in fp64. Computed once per case."""
    ce = n_cls is not None
    params, buffers = O.make_state(0, "RGB", selective, n_cls=n_cls)
    warm, _ = crop_batch(n, h, w, seed=11)
    x, _ = crop_batch(n, h, w, seed=5)
    x = (x * np.float32(gain)).astype(np.float32)
    with torch.no_grad():
        for _ in range(3):
            O.forward(params, buffers, torch.tensor(warm), selective, training=True, ce=ce)
        ref = heads(O.forward(params, buffers, torch.tensor(x), selective, training=False, ce=ce))
        p64 = {k: v.double() for k, v in params.items()}
        b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in buffers.items()}
        ref64 = heads(O.forward(p64, b64, torch.tensor(x).double(), selective, training=False, ce=ce))
    assert float(buffers["decoder_layer_4_1.1.running_mean"].abs().max()) > 0
    return params, buffers, x, ref, ref64


# ----------------------------------------------------------------------------- fixture parity
def test_eval_fixture_parity_split():
    """tests/test_gpu_model.py::test_eval_forward_and_metrics with fp32_eval_path="split": its assertions unchanged."""
    d = G.load("eval_sel_n4_64.npz")
    params, buffers = O.make_state(0, "RGB", True)
    with torch.no_grad():
        for k in buffers:
            if "running" in k:
                buffers[k] = torch.tensor(d["buf/" + k])
        for k in params:
            if "head/" + k in d.files:
                params[k].copy_(torch.tensor(d["head/" + k]))
    net = gpu_net(params, buffers, True, "split")
    assert net.fp32_eval_path == "split" and fp32_eval_conv_path("split") == "split-fp16"
    with recorded_calls() as names:
        o, s, a = gpu_eval(net, d["x"])
    assert "selunet_conv3x3_x2" in names and "selunet_act_amax" in names
    print(f"eval fixture on the split path: output max rel {G.max_rel(o, d['output']):.3e}, selection "
          f"{G.max_rel(s, d['selection']):.3e}")
    assert G.max_rel(o, d["output"]) < 1e-4 and G.max_rel(s, d["selection"]) < 1e-4
    label = d["label"].astype("uint8")
    pred, sel = O.eval_pred_mask(o), O.eval_pred_mask(s)
    ref_pred, ref_sel = d["pred"].astype("uint8"), O.eval_pred_mask(d["selection"])
    flipped = []
    for ours_l, ref_l, ours_m, ref_m in ((o, d["output"], pred, ref_pred), (s, d["selection"], sel, ref_sel)):
        diff = ours_m != ref_m
        err = np.abs(ours_l.astype(np.float64) - ref_l)
        e_meas = float(err[~diff].max(initial=0.0))
        if diff.any():
            worst = float(np.abs(ref_l[diff]).max())
            assert worst <= min(e_meas, 1e-4 * float(np.abs(ref_l).max())), (int(diff.sum()), worst, e_meas)
        flipped.append(diff)
    keep = ~(flipped[0] | flipped[1])
    cm_keep = O.confusion_matrix(label[keep], pred[keep], selection=sel[keep])
    assert np.array_equal(cm_keep, O.confusion_matrix(label[keep], ref_pred[keep], selection=ref_sel[keep]))
    cm = O.confusion_matrix(label, pred, selection=sel)
    assert np.abs(cm - d["eval_cm_selective"]).sum() <= 2 * int((~keep).sum())
    if keep.all():
        assert np.array_equal(cm, d["eval_cm_selective"])
    assert abs(O.miou(cm) - float(d["eval_miou_selective"])) < 0.002


# ----------------------------------------------------------------------------- the path is really taken
def test_split_path_entry_points():
    """split: the split conv and ConvTranspose2d run, the data-driven word once per CBR layer, the training bound
    never; default: none of them; training mode: the same calls whatever the module's eval path says."""
    params, buffers, x, _, _ = oracle_case(2, 64, 64, True)
    xt = torch.tensor(x, device=DEV)
    calls = {}
    for path in ("exact", "split"):
        net = gpu_net(params, buffers, True, path)
        with recorded_calls() as names, torch.no_grad():
            net(xt)
        calls[path] = list(names)
        net.train()
        with recorded_calls() as names:
            o, s, a = net(xt)
            (o.sum() + s.sum() + a.sum()).backward()
        calls["train-" + path] = list(names)
    sp = calls["split"]
    assert sp.count("selunet_conv3x3_x2") >= 10 and sp.count("selunet_gemm_gather_x2") == 3
    assert sp.count("selunet_act_amax") == N_CBR == 14 and "selunet_act_bound" not in sp
    assert not any(n in calls["exact"] for n in SPLIT_ENTRIES)
    assert "selunet_conv3x3_wino" in calls["exact"] or "selunet_gemm_gather" in calls["exact"]
    assert calls["train-exact"] == calls["train-split"]
    assert "selunet_conv3x3_x2" in calls["train-exact"] and "selunet_act_amax" not in calls["train-exact"]
    # everything but the convolutions, the words and their zeroing is the exact path's, in its order
    conv = ("selunet_conv3x3_x2", "selunet_conv3x3_wino", "selunet_gemm_gather", "selunet_gemm_gather_x2",
            "selunet_act_amax", "selunet_memset")
    assert [n for n in sp if n not in conv] == [n for n in calls["exact"] if n not in conv]


def test_attribute_and_unknown_value():
    net = S.UNet_B("RGB", selective=True)
    assert net.fp32_eval_path == "exact"
    net.fp32_eval_path = "split"
    assert net.fp32_eval_path == "split"
    with pytest.raises(ValueError):
        net.fp32_eval_path = "fast"
    assert net.fp32_eval_path == "split"
    assert fp32_eval_conv_path("split", torch.bfloat16) == "bf16"
    # a bf16 module: the request changes nothing, the bf16 kernels run
    params, buffers, x, _, _ = oracle_case(3, 32, 32, True)
    outs = []
    for path in ("exact", "split"):
        net = gpu_net(params, buffers, True, path, dtype=torch.bfloat16)
        with recorded_calls() as names:
            outs.append(gpu_eval(net, x))
        assert not any(n in names for n in SPLIT_ENTRIES)
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


# ----------------------------------------------------------------------------- small shapes against the CPU oracle
CASES = [(3, 32, 32), (1, 40, 48), (2, 64, 64)]


def both_paths(params, buffers, x, selective, n_cls=None):
    out = {}
    for path in ("exact", "split"):
        net = gpu_net(params, buffers, selective, path, n_cls=n_cls)
        with recorded_calls() as names:
            out[path] = gpu_eval(net, x)
        assert ("selunet_conv3x3_x2" in names) == (path == "split")
    return out


def check_against_oracle(tag, out, ref, ref64):
    for i, (r, r64) in enumerate(zip(ref, ref64)):
        e = {p: (G.max_rel(out[p][i], r), G.max_rel(out[p][i], r64)) for p in ("exact", "split")}
        print(f"{tag} head {i}: vs oracle fp32 exact {e['exact'][0]:.3e} split {e['split'][0]:.3e}; vs oracle fp64 "
              f"exact {e['exact'][1]:.3e} split {e['split'][1]:.3e} (oracle fp32 {G.max_rel(r, r64):.3e}); "
              f"split vs exact {G.max_rel(out['split'][i], out['exact'][i]):.3e}")
    for i, r in enumerate(ref):
        assert np.isfinite(out["split"][i]).all()
        assert G.max_rel(out["split"][i], r) < 1e-4, (tag, i)
        assert G.max_rel(out["split"][i], out["exact"][i]) < 1e-4, (tag, i)


@pytest.mark.parametrize("selective", [True, False])
@pytest.mark.parametrize("n,h,w", CASES)
def test_small_shapes_match_oracle(n, h, w, selective):
    """(3, 3, 32, 32): the split conv at 32^2 and 16^2 only; (1, 3, 40, 48): ragged 16x16 tiles at two levels;
    (2, 3, 64, 64). Both against the oracle's fp32 eval forward and against the exact path, 1e-4."""
    params, buffers, x, ref, ref64 = oracle_case(n, h, w, selective)
    out = both_paths(params, buffers, x, selective)
    check_against_oracle(f"eval split ({n}, 3, {h}, {w}) selective={selective}", out, ref, ref64)


def test_ce_unet_matches_oracle():
    params, buffers, x, ref, ref64 = oracle_case(2, 64, 64, True, n_cls=2)
    out = both_paths(params, buffers, x, True, n_cls=2)
    assert out["split"][0].shape == (2, 2, 64, 64)
    check_against_oracle("eval split CE UNet (2, 3, 64, 64)", out, ref, ref64)


# ----------------------------------------------------------------------------- data-driven word
def test_activations_beyond_the_training_bound(monkeypatch):
    """n = 1 at 32 x 32 (M = 1024, sqrt(M) = 32) with the input scaled by 1000: with running statistics the first
    layers' relu(bn(y)) exceed the training-mode word |gamma| sqrt(M) + |beta| (selunet_act_bound's) many times
    over — more than the 4x between the split operand scale (below 2^14) and the fp16 maximum, so fp16 operands scaled
    by that word would overflow. The word taken from the data keeps the forward finite and within the same 1e-4."""
    params, buffers, x, ref, ref64 = oracle_case(1, 32, 32, True, gain=1000.0)
    acts, orig = {}, O._cbr

    def cbr(p, b, name, t, training):
        y = orig(p, b, name, t, training)
        acts[name] = (float(y.max()), y.shape[0] * y.shape[2] * y.shape[3])
        return y
    monkeypatch.setattr(O, "_cbr", cbr)
    with torch.no_grad():
        O.forward(params, buffers, torch.tensor(x), True, training=False)
    monkeypatch.undo()
    ratio = {}
    for name, (amax, m) in acts.items():
        bound = float(params[f"{name}.1.weight"].abs().max()) * m ** 0.5 + float(params[f"{name}.1.bias"].abs().max())
        ratio[name] = amax / bound
    print("max relu(bn(y)) / training bound per layer:", {k: round(v, 2) for k, v in ratio.items()})
    # a layer whose output a split consumer stages (every CBR output but the last feeds a conv or a ConvTranspose2d)
    assert max(v for k, v in ratio.items() if k != "decoder_layer_1_1") > 8
    out = both_paths(params, buffers, x, True)
    check_against_oracle("eval split, input x 1000", out, ref, ref64)


# ----------------------------------------------------------------------------- plan cache
def test_plan_cache_keeps_the_paths_apart():
    params, buffers, x, _, _ = oracle_case(3, 32, 32, True)
    xt = torch.tensor(x, device=DEV)

    def fresh(state, path):
        net = gpu_net(params, buffers, True, path)
        net.load_state_dict(state)
        return gpu_eval(net.eval(), x)

    def same(a, b):
        return all(np.array_equal(p, q) for p, q in zip(a, b))

    net = gpu_net(params, buffers, True, "split")
    s0 = {k: v.clone() for k, v in net.state_dict().items()}
    want = {(0, p): fresh(s0, p) for p in ("exact", "split")}
    assert not same(want[0, "exact"], want[0, "split"])  # (the two paths round differently: a replayed wrong plan shows)
    r1, r1b = gpu_eval(net, x), gpu_eval(net, x)  # recorded, then replayed
    assert same(r1, want[0, "split"]) and same(r1b, r1)
    net.fp32_eval_path = "exact"
    assert same(gpu_eval(net, x), want[0, "exact"])
    net.train()  # a training step: running statistics and parameters move
    opt = S.Adam(net.parameters(), lr=1e-3)
    o, s, a = net(xt)
    (o.mean() + s.mean() + a.mean()).backward()
    opt.step()
    net.eval()
    s1 = {k: v.clone() for k, v in net.state_dict().items()}
    assert not torch.equal(s1["encoder_layer_1_2.1.running_mean"], s0["encoder_layer_1_2.1.running_mean"])
    want.update({(1, p): fresh(s1, p) for p in ("exact", "split")})
    assert same(gpu_eval(net, x), want[1, "exact"])
    net.fp32_eval_path = "split"
    r4, r4b = gpu_eval(net, x), gpu_eval(net, x)
    assert same(r4, want[1, "split"]) and same(r4b, r4) and not same(r4, r1)
    net.fp32_eval_path = "exact"
    assert same(gpu_eval(net, x), want[1, "exact"])


# ----------------------------------------------------------------------------- fallback
CHILD = """
import numpy as np, torch
from tests import test_gpu_eval_split as T
from selectivenet_for_semantic_segmentation_binary_amd.engine import fp32_eval_conv_path
params, buffers, x, _, _ = T.oracle_case(3, 32, 32, True)
assert fp32_eval_conv_path("split").startswith("exact-fp32")
outs = []
for path in ("exact", "split"):
    net = T.gpu_net(params, buffers, True, path)
    with T.recorded_calls() as names:
        outs.append(T.gpu_eval(net, x))
    assert names and not any(n in names for n in T.SPLIT_ENTRIES), names
assert all(np.array_equal(a, b) for a, b in zip(*outs))
print("FALLBACK-OK")
"""


def test_split_request_without_x2_is_the_exact_path():
    """SELUNET_X2=0 (read when the engine is made: a fresh process): a "split" request calls no split entry point and
    is bit-identical to "exact"; fp32_eval_conv_path says so."""
    env = dict(os.environ, SELUNET_X2="0", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FALLBACK-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ----------------------------------------------------------------------------- eval CLI
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("eval_split_cli")
    ck = tmp / "checkpoint"
    ck.mkdir()
    lab = calibrated_checkpoint(ck / "model_epoch1.pth")
    base = ["--data_dir", "synthetic:8", "--patch_size", "64", "--test_fold", "2", "--model_dir", str(ck),
            "--model_arch", "UNet_B", "--selective", "1", "--batch_size", "4", "--select_eval", "1"]

    def run(name, *extra):
        out = tmp / name
        res = EV.evaluate(EV.parse_arguments(base + ["--save_dir", str(out)] + list(extra)))
        return res, out

    logits = {}
    ds = D.PatchSet(*D.load_test_set_for_tests("synthetic:8", 64, 2))
    for path in ("exact", "split"):
        net = S.UNet_B("RGB", selective=True, fp32_eval_path=path)
        net_utils.net_test_load(str(ck / "model_epoch1.pth"), net)
        net = net.to(DEV).train(False)
        loader = D.BatchLoader(ds, 4, shuffle=False, random_flip=False, device=torch.device(DEV, 0), input_type="RGB")
        o_s = [gpu_eval_t(net, x) for x, _ in loader]
        logits[path] = [np.concatenate([b[i] for b in o_s]) for i in (0, 1)]
    return {"lab": lab, "logits": logits, "exact": run("exact"), "split": run("split", "--fp32_path", "split"),
            "split_report": run("split_report", "--fp32_path", "split", "--s_cut_off_steps", "4", "--patch_report", "1")}


def gpu_eval_t(net, xt):
    with torch.no_grad():
        return heads(net(xt))


def test_eval_cli_split_confusion_matrix(cli):
    """performance.json of --fp32_path split against the default run: the matrices differ by at most the pixels whose
    exact-path logit lies within the measured logit error of a cut-off (the flip rule of the fixture test)."""
    ex, sp = cli["logits"]["exact"], cli["logits"]["split"]
    flipped = np.zeros(ex[0].shape, bool)
    for e, s in zip(ex, sp):
        diff = O.eval_pred_mask(e) != O.eval_pred_mask(s)
        err = np.abs(s.astype(np.float64) - e)
        e_meas = float(err[~diff].max(initial=0.0))
        print(f"eval CLI logits, split vs exact: max rel {G.max_rel(s, e):.3e}, {int(diff.sum())} mask bits differ")
        assert G.max_rel(s, e) < 1e-4
        if diff.any():
            worst = float(np.abs(e[diff]).max())
            assert worst <= min(e_meas, 1e-4 * float(np.abs(e).max())), (int(diff.sum()), worst, e_meas)
        flipped |= diff
    cm_e = np.array(json.load(open(cli["exact"][1] / "performance.json"))["confusion_matrix"])
    cm_s = np.array(json.load(open(cli["split"][1] / "performance.json"))["confusion_matrix"])
    assert cm_e.sum() > 0 and np.abs(cm_s - cm_e).sum() <= 2 * int(flipped.sum())
    if not flipped.any():
        assert np.array_equal(cm_s, cm_e)
    # the CLI's matrix is the one of the split-path logits obtained here
    lab = cli["lab"].astype("uint8")
    want = O.confusion_matrix(lab, O.eval_pred_mask(sp[0]), selection=O.eval_pred_mask(sp[1]))
    assert np.array_equal(cm_s, want)
    assert abs(cli["split"][0]["mIoU"] - cli["exact"][0]["mIoU"]) < 0.002


def test_eval_cli_split_with_sweep_and_patch_report(cli):
    res, out = cli["split_report"]
    assert res["confusion_matrix"] == cli["split"][0]["confusion_matrix"]
    rows = res["patch_report"]["rows"]
    assert len(rows) == 8
    cm = [[sum(r["sel_cm00"] for r in rows), sum(r["sel_cm01"] for r in rows)],
          [sum(r["sel_cm10"] for r in rows), sum(r["sel_cm11"] for r in rows)]]
    assert cm == res["confusion_matrix"]
    curve = res["risk_coverage"]["curve"]
    assert [r["s_cut_off"] for r in curve] == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert curve[2]["confusion_matrix"] == res["confusion_matrix"]
    for f in ("performance.json", "risk_coverage.json", "patch_performance.csv"):
        assert (out / f).exists()


def test_eval_cli_printed_line(cli, capsys):
    base = ["--data_dir", "synthetic:8", "--patch_size", "64", "--test_fold", "2", "--model_dir",
            str(cli["exact"][1].parent / "checkpoint"), "--selective", "1", "--batch_size", "4", "--save_dir",
            str(cli["exact"][1].parent / "main")]
    EV.main(base + ["--fp32_path", "split"])
    on = capsys.readouterr().out
    assert "fp32_path='split'" in on


# ----------------------------------------------------------------------------- train CLI
def test_train_cli_valid_fp32_path(tmp_path):
    """One short epoch with --val_steps 1, with and without --valid_fp32_path split: the training loss identical
    (training forwards never look at the flag), the validation loss to 1e-4 relative."""
    hist = {}
    for path in ("exact", "split"):
        argv = ["--data_dir", "synthetic:40", "--patch_size", "64", "--model_arch", "UNet_B", "--loss", "BCElogit",
                "--selective", "1", "--batch_size", "8", "--model_dir", str(tmp_path / path), "--steps_per_epoch", "2",
                "--val_steps", "1", "--n_epoch", "1", "--quiet"] + (["--valid_fp32_path", "split"] if path == "split" else [])
        args = TR.parse_arguments(argv)
        with recorded_calls() as names:
            h = TR.train(args, str(tmp_path / path / "ck"), str(tmp_path / path / "log"))
        assert ("selunet_act_amax" in names) == (path == "split")
        hist[path] = h[0]
    a, b = hist["exact"], hist["split"]
    print(f"train CLI: train loss {a['train_loss']!r} / {b['train_loss']!r}, valid loss {a['valid_loss']!r} / "
          f"{b['valid_loss']!r}")
    assert a["train_loss"] == b["train_loss"] and a["train_cm"] == b["train_cm"]
    assert abs(a["valid_loss"] - b["valid_loss"]) <= 1e-4 * abs(a["valid_loss"])
