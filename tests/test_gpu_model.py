"""End-to-end parity of the MI355X SelectiveUNet_B training step against the reference.

The expected values are the golden fixtures produced by running the reference's own model.py /
selective_loss.py / torch Adam (tests/golden/make_golden.py). Step 0 is compared at the
north-star tolerance (1e-4 fp32 on logits and loss, bit-exact prediction masks) and the
gradients against the reference's own fp64 run (no worse than the reference's fp32 error);
later steps loosely, for the reason given in tests/test_oracle.py::_run_oracle_fixture.
"""
import hashlib

import numpy as np
import pytest
import torch

import selectivenet_for_semantic_segmentation_binary_amd as S
import selectivenet_for_semantic_segmentation_binary_amd.layout as L
from oracle import unet_b_cpu as O
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd.engine import fp32_conv_path
from selectivenet_for_semantic_segmentation_binary_amd.synthetic import make_batch
from tests import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRE_BN_BIAS = {f"{n}.0.bias" for n, _, _ in L.CBR_LAYERS}
# relative L2 gradient error against the reference's fp32 run, for fixtures without an fp64 truth
REF32_GRAD_BOUND = 1e-4


def build(selective, seed=0, dtype=torch.float32):
    net = S.UNet_B("RGB", selective=selective, compute_dtype=dtype)
    p = L.seeded_params(seed, "RGB", selective)
    with torch.no_grad():
        for k, t in net.named_parameters():
            t.copy_(torch.tensor(p[k]))
    return net.to(DEV).train()


def train_step(net, opt, x, lab, selective, lamb, chunks=1):
    """train.py:194-209 on the MI355X path (DataParallel chunk semantics emulated in one
    process when chunks > 1: per-chunk BN, replica-0 buffers kept, loss on the whole batch)."""
    loss_A = S.BCEWithLogitsLoss()
    outs, saved = [], None
    for r, xc in enumerate(torch.chunk(x, chunks)):
        o = net(xc)
        outs.append(o if selective else (o,))
        if chunks > 1 and r == 0:
            saved = {k: v.clone() for k, v in net.named_buffers()}
    if saved is not None:
        with torch.no_grad():
            for k, v in net.named_buffers():
                v.copy_(saved[k])
    output = torch.cat([o[0] for o in outs])
    res = {}
    if selective:
        sel = torch.cat([o[1] for o in outs])
        aux = torch.cat([o[2] for o in outs])
        aux_loss = loss_A(aux, lab)
        select_loss, coverage = S.calc_selective_risk_image_b(output, sel, target=lab, lamb=lamb)
        loss = aux_loss + select_loss
        res.update(coverage=coverage.item(), aux_loss=aux_loss.item(), select_loss=select_loss.item(),
                   selection=sel.detach().cpu().numpy(), aux=aux.detach().cpu().numpy())
    else:
        loss = loss_A(output, lab)
    opt.zero_grad()
    loss.backward()
    res["grads"] = {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters()}
    opt.step()
    res.update(loss=loss.item(), output=output.detach().cpu().numpy())
    return res


def check_step(d, s, r, strict, info=None):
    """Compare one training step's results `r` (loss, coverage, output, grads, params, buffers,
    num_batches_tracked — numpy) with step `s` of golden fixture `d`; returns failure strings.
    info (step 0): filled with the loss's relative error, the worst gradient relative L2 error and
    the number of flipped prediction-mask pixels."""
    selective = bool(d["meta_selective"])
    pre = f"s{s}/"
    # later steps (after one or more Adam steps): the loss to 1e-4 relative, logits to 5e-3 — measured
    # 3e-6..1.5e-5 and 0.9e-3..1.8e-3 (profiles/r05k_later_steps.txt): Adam moves an element whose gradient
    # sits at rounding level by +-lr either way, which the logits see at the 1e-3 level; the loss averages it
    tol = 1e-4 if strict else 1e-4
    tol_logits = 1e-4 if strict else 5e-3
    ref_loss = float(d[pre + "loss"])
    if info is not None:
        info["loss_rel_err"] = abs(r["loss"] - ref_loss) / max(1e-30, abs(ref_loss))
    if not strict:  # (the later steps' measured deviation, for the record)
        out_ref = d[pre + "output"] if pre + "output" in d.files else d[pre + "output_val"]
        out_got = r["output"] if pre + "output" in d.files else r["output"].ravel()[d[pre + "output_idx"]]
        print(f"{pre} loss rel err {abs(r['loss'] - ref_loss) / max(1e-30, abs(ref_loss)):.2e}, "
              f"logits max rel {G.max_rel(out_got, out_ref):.2e}" +
              "".join(f", {h} max rel {G.max_rel(r[h], d[pre + h]):.2e}" for h in ("selection", "aux")
                      if h in r and pre + h in d.files))
    assert abs(r["loss"] - ref_loss) <= tol * max(1.0, abs(ref_loss)), (s, r["loss"], ref_loss)
    if selective:
        assert abs(r["coverage"] - float(d[pre + "coverage"])) <= tol
        for k in ("aux_loss", "select_loss"):
            assert abs(r[k] - float(d[pre + k])) <= tol * max(1.0, abs(float(d[pre + k]))), (k, r[k])
    if pre + "output" in d.files:
        assert G.max_rel(r["output"], d[pre + "output"]) < tol_logits
    else:
        flat = r["output"].ravel()
        assert G.max_rel(flat[d[pre + "output_idx"]], d[pre + "output_val"]) < tol_logits
    for h in ("selection", "aux"):
        if h in r and pre + h in d.files:
            assert G.max_rel(r[h], d[pre + h]) < tol_logits, h
        elif h in r and pre + h + "_idx" in d.files:
            assert G.max_rel(r[h].ravel()[d[pre + h + "_idx"]], d[pre + h + "_val"]) < tol_logits, h
    fails = []
    if strict:
        # prediction masks (train.py:150,153): report the flipped pixels; none may flip unless a
        # reference logit lies within 1e-6 of the boundary, and any flip must sit within the
        # logit tolerance of it
        mask = O.train_pred_mask(r["output"])
        same = hashlib.sha1(mask.tobytes()).hexdigest() == d[pre + "output_mask_sha1"].item().decode()
        flips, near0 = (0, None) if same else G.mask_flips(d, pre, "output", r["output"], tol)
        print(f"{pre}output mask: {flips} flipped pixels of {mask.size} "
              f"(reference logits within 1e-6 of the boundary: {near0 if near0 is not None else 'n/a'})")
        if info is not None:
            info["mask_flips"], info["near0"] = flips, near0
        if not same and near0 == 0:
            assert flips == 0, f"{flips} mask pixels flipped with no reference logit within 1e-6 of the boundary"
    if s == 0 and any(k.startswith("s0/grad64norm/") for k in d.files):
        # gradients: no worse than the reference's own fp32 error against its fp64 run
        f, report = G.check_grads_vs_truth(d, r["grads"], skip=PRE_BN_BIAS)
        print("worst grad errors vs fp64 (ours, reference fp32, perturbed reference):",
              [(n, f"{a:.1e}", f"{b:.1e}", f"{c:.1e}") for n, a, b, c in report[:6]])
        if info is not None:
            info["worst_grad"] = (report[0][0], report[0][1], "vs reference fp64")
        fails += f
    elif s == 0:
        # no fp64 run (batch 128 at 256x256 would need ~170 GB of host memory): against the
        # reference's fp32 gradients directly (REF32_GRAD_BOUND)
        f, report = G.check_grads_vs_ref32(d, r["grads"], REF32_GRAD_BOUND, skip=PRE_BN_BIAS)
        print("worst grad errors vs reference fp32 (samples, norm, reference spread):",
              [(n, f"{a:.1e}", f"{b:.1e}", f"{c:.1e}") for n, a, b, c in report[:6]])
        if info is not None:
            info["worst_grad"] = (report[0][0], report[0][1], "vs reference fp32")
        fails += f
    if s == 0:
        # pre-BN conv biases cancel inside training-mode BN: their gradient is 0 up to rounding on
        # both sides (fp64: ~1e-16) — ours may be no larger than the reference's own noise
        for k in PRE_BN_BIAS & set(r["grads"]):
            ref = d[pre + "gradfull/" + k] if pre + "gradfull/" + k in d.files else d[pre + "gradval/" + k]
            got = np.abs(r["grads"][k]).max()
            if got > max(1e-6, 4 * np.abs(ref).max()):
                fails.append(f"{k}: |grad| {got:.2e} > rounding level (reference {np.abs(ref).max():.2e})")
    # (after one Adam step every element has moved by ~lr*sign(g); elements whose gradient
    # sits within rounding of zero move either way, so later-step gradients are not compared
    # element-wise — loss, logits, parameters and BN buffers are, loosely)
    # Adam moves an element by ~lr*sign(g); elements whose gradient sits at rounding level
    # (pre-BN biases, near-tie ReLU/max-pool routes) can move the other way: floor 2.5*lr.
    fails += G.check_tensors(d, pre + "param", r["params"], rtol=1e-5, atol=2.5e-3 if strict else 5e-3)
    for k, v in r["buffers"].items():
        if "running" in k:
            at = 1e-5 if strict else 3e-3
            np.testing.assert_allclose(v, d[pre + "buf/" + k], rtol=1e-4 if strict else 1e-2, atol=at, err_msg=k)
    assert int(r["num_batches_tracked"]) == int(d[pre + "num_batches_tracked"])
    return fails


def run_fixture(fname, strict_steps=1):
    """Run fixture `fname` through the HIP path and check every step (check_step). Returns the
    step-0 summary (loss error, worst gradient error, mask flips) and records it in G.SUMMARY
    (printed at the end of the pytest run by tests/conftest.py)."""
    d = G.load(fname)
    n, size = int(d["meta_n"]), int(d["meta_size"])
    selective = bool(d["meta_selective"])
    x, lab = make_batch(n, size, seed=int(d["meta_data_seed"]))
    assert hashlib.sha1(x.tobytes()).hexdigest() == d["x_sha1"].item().decode()
    net = build(selective, int(d["meta_seed"]))
    opt = S.Adam(net.parameters(), lr=1e-3)
    xt, lt = torch.tensor(x, device=DEV), torch.tensor(lab, device=DEV)
    fails, info = [], {}
    for s in range(int(d["meta_steps"])):
        r = train_step(net, opt, xt, lt, selective, int(d["meta_lamb"]), int(d["meta_chunks"]))
        r["params"] = {k: p.detach().cpu().numpy() for k, p in net.named_parameters()}
        bufs = dict(net.named_buffers())
        r["buffers"] = {k: v.cpu().numpy() for k, v in bufs.items()}
        r["num_batches_tracked"] = int(bufs["encoder_layer_1_1.1.num_batches_tracked"])
        fails += check_step(d, s, r, strict=s < strict_steps, info=info if s == 0 else None)
    info["path"] = fp32_conv_path()
    info["fixture"] = fname
    G.SUMMARY.append(G.format_summary(info))
    assert not fails, "\n".join(fails[:25])
    return info


@pytest.mark.parametrize("fname", ["step_sel_n2_64.npz", "step_nosel_n2_64.npz", "step_sel_lamb8_n3_32.npz",
                                   "dp_sel_n8_32_c4.npz"])
def test_train_step_matches_reference(fname):
    run_fixture(fname)


def test_train_step_full_size_256():
    run_fixture("step_sel_n4_256.npz")


def test_eval_forward_and_metrics():
    """net.eval() forward (eval.py:156,203-205) with running statistics, eval masks (fp32 sigmoid
    > 0.5, eval.py:175,179) and the Evaluator confusion matrix / mIoU (compute_metric.py:10-65)."""
    d = G.load("eval_sel_n4_64.npz")
    net = build(True)
    with torch.no_grad():
        for k, v in net.named_buffers():
            if "running" in k:
                v.copy_(torch.tensor(d["buf/" + k]))
        for k, p in net.named_parameters():
            if "head/" + k in d.files:
                p.copy_(torch.tensor(d["head/" + k]))
    net.eval()
    with torch.no_grad():
        o, s, a = net(torch.tensor(d["x"], device=DEV))
    o, s = o.cpu().numpy(), s.cpu().numpy()
    assert G.max_rel(o, d["output"]) < 1e-4 and G.max_rel(s, d["selection"]) < 1e-4
    # eval masks (fp32 sigmoid > 0.5) of both heads; a mask bit may differ from the reference's only where
    # the reference logit lies within the logit error this run measures on the other pixels (the
    # training steps' rule, tests/_golden.py::mask_flips), capped at 1e-4 of the largest |logit|
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
    # the confusion matrix is compared in every case: over the pixels outside the allowed flips it must be
    # the reference's exactly; with no flips that is the fixture's whole selective matrix and mIoU
    cm_keep = O.confusion_matrix(label[keep], pred[keep], selection=sel[keep])
    assert np.array_equal(cm_keep, O.confusion_matrix(label[keep], ref_pred[keep], selection=ref_sel[keep]))
    cm = O.confusion_matrix(label, pred, selection=sel)
    assert np.abs(cm - d["eval_cm_selective"]).sum() <= 2 * int((~keep).sum())
    if keep.all():
        assert np.array_equal(cm, d["eval_cm_selective"])
    assert abs(O.miou(cm) - float(d["eval_miou_selective"])) < 0.002


def test_bf16_step_tracks_fp32():
    """bf16 operands / fp32 accumulation (the speed configuration): same loss to ~1e-2 and gradient
    directions aligned with the fp32 path."""
    d = G.load("step_sel_n2_64.npz")
    x, lab = make_batch(2, 64, seed=int(d["meta_data_seed"]))
    xt, lt = torch.tensor(x, device=DEV), torch.tensor(lab, device=DEV)
    res = {}
    for dt in (torch.float32, torch.bfloat16):
        net = build(True, dtype=dt)
        opt = S.Adam(net.parameters(), lr=1e-3)
        res[dt] = train_step(net, opt, xt, lt, True, 2)
    a, b = res[torch.float32], res[torch.bfloat16]
    assert abs(a["loss"] - b["loss"]) < 2e-2 * abs(a["loss"])
    for k in a["grads"]:
        if k in PRE_BN_BIAS:
            continue
        ga, gb = a["grads"][k].ravel().astype(np.float64), b["grads"][k].ravel().astype(np.float64)
        cos = ga @ gb / (np.linalg.norm(ga) * np.linalg.norm(gb) + 1e-30)
        assert cos > 0.8, (k, cos)


def test_adam_matches_reference_algorithm():
    torch.manual_seed(0)
    ps = [torch.randn(n, device=DEV) for n in (5, 4096, 10000)]
    ref = [p.detach().cpu().clone().requires_grad_() for p in ps]
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = S.Adam(params, lr=1e-2, weight_decay=0.01)
    ropt = torch.optim.Adam(ref, lr=1e-2, weight_decay=0.01)
    for step in range(3):
        for p, r in zip(params, ref):
            g = torch.randn(p.shape) * (step + 1)
            p.grad = g.to(DEV)
            r.grad = g.clone()
        opt.step()
        ropt.step()
    for p, r in zip(params, ref):
        assert torch.allclose(p.detach().cpu(), r.detach(), rtol=1e-6, atol=1e-6)
    sd = opt.state_dict()
    ropt2 = torch.optim.Adam([r.detach().clone().requires_grad_() for r in ref], lr=1e-2)
    ropt2.load_state_dict(sd)  # checkpoint interchangeability (utils/net_utils.py:5-9)


class _conv_noise:
    """Context: the oracle module's conv2d / conv_transpose2d outputs get out + out * eps * N(0, 1)
    (member-seeded) — the conv-output noise ensemble of tests/golden/make_golden.py."""

    def __init__(self, mod, eps, member):
        self.mod, self.eps, self.gen = mod, eps, torch.Generator().manual_seed(5000 + member)

    def _wrap(self, fn):
        def f(*a, **kw):
            out = fn(*a, **kw)
            z = torch.randn(out.shape, generator=self.gen, dtype=torch.float64).to(out.dtype)
            return out + out * (self.eps * z)
        return f

    def __enter__(self):
        import types
        self.F = self.mod.F
        ns = types.SimpleNamespace(**{k: getattr(self.F, k) for k in dir(self.F) if not k.startswith("__")})
        ns.conv2d, ns.conv_transpose2d = self._wrap(self.F.conv2d), self._wrap(self.F.conv_transpose2d)
        self.mod.F = ns
        return self

    def __exit__(self, *exc):
        self.mod.F = self.F


@pytest.mark.parametrize("input_type,n,h,w,selective", [
    ("GH", 2, 32, 32, True),     # model.py:24-27: 'GH' inputs have 2 channels
    ("RGB", 1, 32, 48, True),    # batch of one, non-square patches
    ("RGB", 3, 48, 32, False),   # non-selective UNet_B, odd batch, non-square
])
def test_step_against_oracle_shapes(input_type, n, h, w, selective):
    """One fp32 training step (forward, losses, backward) against the CPU oracle at shapes the
    fixtures do not cover. Loss within 1e-4 relative of the oracle's fp32 run; gradients judged
    as in check_step: relative-L2 error against the oracle's fp64 run within tests/_golden.grad_bound
    of the oracle fp32 run's own error (ReLU / max-pool near-ties route fp32
    gradients differently under any change of summation order)."""
    step_against_oracle(input_type, n, h, w, selective, L.seeded_params(3, input_type, selective))


def test_step_against_oracle_nonpersistent_halo():
    """test_step_against_oracle_shapes at 2x32x32 with SELUNET_OPT_HALO_PERSIST = 0, set before the net (and so
    its engine) is built and restored after: selunet_conv3x3_x2_ok / _wino_ok answer 0, every halo-sized 3x3
    layer falls back to conv3x3_halo<f32,BN> with one statistics row per 16x16 tile, and the engine has to size
    its slabs from the queries for the step to come out right. Same bounds as that test."""
    prev = K.set_option("HALO_PERSIST", 0)
    try:
        assert K.query("selunet_conv3x3_x2_ok", 32, 32, 64, 64, 64) == 0
        step_against_oracle("RGB", 2, 32, 32, True, L.seeded_params(3, "RGB", True))
    finally:
        K.set_option("HALO_PERSIST", prev)


def drifted_params(input_type, selective, seed=77):
    """A parameter state as training leaves it, from one numpy recipe for the net and the oracle: every BN gamma
    ~ N(0, 1) with 5 % exact zeros, every BN beta ~ N(0, 0.5), every 3x3 conv weight row scaled by 2^U(-6, 6) (the
    per-row scales of the split-fp16 weight pack; large and small batch variances)."""
    p = L.seeded_params(3, input_type, selective)
    rng = np.random.Generator(np.random.PCG64(seed))
    for name, _, co in L.CBR_LAYERS:
        gamma = rng.standard_normal(co)
        gamma[rng.random(co) < 0.05] = 0.0
        p[f"{name}.1.weight"] = gamma.astype(np.float32)
        p[f"{name}.1.bias"] = (0.5 * rng.standard_normal(co)).astype(np.float32)
        w = p[f"{name}.0.weight"]
        p[f"{name}.0.weight"] = (w * 2.0 ** rng.uniform(-6, 6, size=(co, 1, 1, 1))).astype(np.float32)
    return p


_ORACLE_CACHE = {}


@pytest.mark.parametrize("input_type,n,h,w,selective", [
    ("RGB", 2, 32, 32, True),
    ("RGB", 2, 40, 56, True),    # pyramid 40x56, 20x28, 10x14, 5x7: split-fp16 eligibility flips, ragged tiles
    ("RGB", 3, 24, 24, False),
    ("RGB", 1, 64, 136, True),   # deepest level 8x17: the odd width puts decoder_layer_4_x's exact-fp32 weight
                                 # gradient on the fp32 halo kernel's split partials (no Winograd pairs)
])
@pytest.mark.parametrize("x2", ["1", "0"])  # the default split-fp16 path, the exact-fp32 path
def test_step_against_oracle_drifted_state(input_type, n, h, w, selective, x2, monkeypatch):
    """test_step_against_oracle_shapes from a drifted parameter state (drifted_params: BN gammas of both signs
    and exactly zero, betas of either sign, conv rows over a 2^12 range of scales) instead of the seeded one
    (gamma in [0.6, 1.4]), with the same bounds, and the running statistics after the step against the oracle's
    (rtol 1e-4, atol 1e-5, as check_step's strict step). The oracle's own fp32 and fp64 runs agree on this
    state to rounding except where one ReLU / max-pool kink flips, which grad_bound's ensemble terms absorb."""
    monkeypatch.setenv("SELUNET_X2", x2)  # read when the engine is built
    step_against_oracle(input_type, n, h, w, selective, drifted_params(input_type, selective), buffers=True,
                        cache_key=("drifted", input_type, n, h, w, selective))


def step_against_oracle(input_type, n, h, w, selective, p, buffers=False, cache_key=None):
    """One training step of the HIP path from parameters p (key -> ndarray) against the oracle from the same p."""
    x, lab = make_batch(n, max(h, w), seed=11)
    x = np.ascontiguousarray(x[:, :L.input_channels(input_type), :h, :w])
    lab = np.ascontiguousarray(lab[:, :h, :w])
    net = S.UNet_B(input_type, selective=selective)
    with torch.no_grad():
        for k, t in net.named_parameters():
            t.copy_(torch.tensor(p[k]))
    net = net.to(DEV).train()
    xt, lt = torch.tensor(x, device=DEV), torch.tensor(lab, device=DEV)
    outs = net(xt)
    if selective:
        out, sel, aux = outs
        sl, _ = S.calc_selective_risk_image_b(out, sel, lt, lamb=2)
        loss = S.BCEWithLogitsLoss()(aux, lt) + sl
    else:
        loss = S.BCEWithLogitsLoss()(outs, lt)
    loss.backward()
    torch.cuda.synchronize()

    obuf = {}

    def oracle(dt, xin=x):
        params, bufs = O.make_state(3, input_type, selective)
        params = {k: torch.tensor(p[k]).to(dt).requires_grad_() for k in params}
        bufs = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in bufs.items()}
        xo, lo = torch.tensor(xin, dtype=dt), torch.tensor(lab, dtype=dt)
        ro = O.forward(params, bufs, xo, selective, training=True)
        obuf[dt] = bufs
        if selective:
            o2, s2, a2 = ro
            sl2, _ = O.selective_risk_b_stable(o2, s2, lo, lamb=2)
            l2 = O.bce_with_logits_mean(a2, lo) + sl2
        else:
            l2 = O.bce_with_logits_mean(ro, lo)
        l2.backward()
        return float(l2.detach()), {k: v.grad.double() for k, v in params.items()}

    if cache_key in _ORACLE_CACHE:  # (the same reference for both convolution paths)
        loss32, g32, g64, ens, b32 = _ORACLE_CACHE[cache_key]
    else:
        loss32, g32, g64, ens, b32 = oracle_reference(oracle, obuf, x)
        if cache_key is not None:
            _ORACLE_CACHE[cache_key] = (loss32, g32, g64, ens, b32)
    assert abs(loss.item() - loss32) < 1e-4 * max(1.0, abs(loss32))
    fails = []
    for k, q in net.named_parameters():
        if k in PRE_BN_BIAS:  # cancels inside training-mode BN: zero gradient on both sides
            continue
        assert bool(torch.isfinite(q.grad).all()), k
        nrm = float(g64[k].norm()) + 1e-30
        err = float((q.grad.cpu().double() - g64[k]).norm()) / nrm
        err_ref = float((g32[k] - g64[k]).norm()) / nrm
        if not err <= G.grad_bound(err_ref, ens[k]):
            fails.append((k, err, err_ref, ens[k]))
    assert not fails, fails
    if buffers:
        for k, v in net.named_buffers():
            if "running" in k:
                np.testing.assert_allclose(v.cpu().numpy(), b32[k].numpy(), rtol=1e-4, atol=1e-5, err_msg=k)


def oracle_reference(oracle, obuf, x):
    """The oracle's fp32 loss and gradients, its fp64 gradients, its own fp32 error under rounding-level
    perturbations (the e_ens of tests/_golden.grad_bound) and its buffers after the unperturbed fp32 step."""
    loss32, g32 = oracle(torch.float32)
    b32 = {k: v.clone() for k, v in obuf[torch.float32].items()}
    _, g64 = oracle(torch.float64)
    # the oracle's own fp32 error on 4 rounding-level perturbations of the input (the e_ens of
    # tests/_golden.grad_bound)
    ens = {}
    for m in range(1, 5):
        rng = np.random.Generator(np.random.PCG64(1000 + m))
        xp = (x.astype(np.float64) * (1.0 + 1e-7 * rng.standard_normal(x.shape))).astype(np.float32)
        _, p32 = oracle(torch.float32, xp)
        _, p64 = oracle(torch.float64, xp)
        for k in p64:
            ens[k] = max(ens.get(k, 0.0), float((p32[k] - p64[k]).norm() / (p64[k].norm() + 1e-30)))
    # ... and with rounding-level noise on every convolution output (3e-7 relative: the measured
    # rounding of the fp32 Winograd F(2,3) convolution against fp64; make_golden.py::
    # augment_conv_noise), against the unperturbed fp64 run. At 3x48x32 (non-selective) one ReLU
    # input of encoder_layer_2_x sits within that noise of zero: 2 of 16 oracle members flip it and
    # land at 7.36e-4 on encoder_layer_2_1.0.weight — as does the HIP path; none flips at 2e-7.
    for m in range(1, 9):
        with _conv_noise(O, 3e-7, m):
            _, p32 = oracle(torch.float32)
        for k in g64:
            ens[k] = max(ens[k], float((p32[k] - g64[k]).norm() / (g64[k].norm() + 1e-30)))
    return loss32, g32, g64, ens, b32
