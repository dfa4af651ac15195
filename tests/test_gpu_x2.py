"""fp32 3x3 convolution on split-fp16 operands (selunet_conv3x3_x2, conv3x3_halo_persist_kernel
<float, BN, X2>) against torch's conv2d / conv2d input gradient in fp64 on the CPU: the weight pack
(SELUNET_PACK_CONV3X3_X2), forward with the BN-statistics epilogue and torch.cat sources with folded
BN+ReLU staging, data gradient with the split (ConvTranspose bias column sums) and BN-backward-sums
epilogues, and the operand range words (selunet_act_bound, selunet_bn_bwd_apply_amax, the
epilogue's amax).

Tolerance: 2e-6 of the tensor's max magnitude against the fp64 result, as the fp32 Winograd kernel
(tests/test_gpu_wino.py): v*2^e = h + l holds 22 significant bits per operand and the three fp16
products are summed in fp32 accumulators 16 at a time, measured at or below the exact fp32 MFMA's
error (tools/split_probe.hip: relative RMS 3.8e-7 vs 4.3e-7 at K = 1152)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from tests.test_gpu_kernels import (bn_fold, bnb_operands, check_bnb_sums, check_signed_inputs,  # noqa: F401
                                    gather_wgs, gen, halo_wgs, nchw, nhwc, rel, signed_gamma)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-6
# Range words as training passes them: every input word multiplied by `slack`. A BN+ReLU source's word is the
# Samuelson bound |gamma| sqrt(M) + |beta| (selunet_act_bound), 2^9..2^10 above the real maximum at 128 x 256^2,
# so operands sit that much lower in the fp16 range. TOL stays: tests/test_split_emulation.py bounds the
# operand-only error of the split at 2e-7 up to slack 2^12.
SLACKS = [2.0 ** 10, 2.0 ** 12]


@pytest.fixture
def x2d():
    """Set SELUNET_OPT_X2D for one test (1: every 64-column layer on conv3x3_x2d_kernel, 0: none)."""
    prev = []

    def setter(mode):
        prev.append(K.set_option("X2D", mode))
    yield setter
    for v in prev[:1]:
        K.set_option("X2D", v)


@pytest.fixture
def tile_queue():
    """The 128-column kernel variant for one test: 0 the static persistent walk, 1 SELUNET_OPT_TILE_QUEUE (tiles
    from a ticket counter, statistics per tile), 2 SELUNET_OPT_X2P (conv3x3_x2p_kernel: two 256-thread workgroups
    per CU, LDS-DMA weights; default off, measured slower — kept tested)."""
    prev = []

    def setter(mode):
        prev.append((K.set_option("TILE_QUEUE", 1 if mode == 1 else 0), K.set_option("X2P", 1 if mode == 2 else 0)))
    yield setter
    for tq, xp in prev[:1]:
        K.set_option("TILE_QUEUE", tq)
        K.set_option("X2P", xp)


def pack_x2(w, dgrad=True):
    """Split-fp16 operands of a conv3x3 weight [co][ci][3][3] through selunet_pack_weights: fwd
    [co][9*ci] words + co unscale factors, dgrad [ci][9*co] + ci."""
    co, ci = w.shape[:2]
    wd = w.to(DEV).contiguous()
    fwd = torch.empty(co * 9 * ci + co, device=DEV)
    dg = torch.empty(ci * 9 * co + ci, device=DEV) if dgrad else None
    pl = K.PackList()
    pl.d[0] = K.PackDesc(K.ptr(wd), K.ptr(fwd), K.ptr(dg), K.PACK_CONV3X3_X2, co, ci, 9 * ci, 0)
    pl.n = 1
    K.call("selunet_pack_weights", pl, K.F32, K.stream_ptr())
    return fwd, dg


def unpack_x2(buf, rows, k):
    """fp64 [rows][k] matrix a split-fp16 pack holds: (h + l) * unscale."""
    m = buf[: rows * k].cpu().view(torch.float16).reshape(rows, k // 32, 2, 32).double()
    v = (m[:, :, 0] + m[:, :, 1]).reshape(rows, k)
    return v * buf[rows * k:].cpu().double().view(rows, 1)


def test_x2_pack():
    w = gen(64, 96, 3, 3, seed=1, scale=0.1)
    w[3] *= 1e-3  # rows of very different ranges: one scale per row
    fwd, dg = pack_x2(w)
    torch.cuda.synchronize()
    ref_f = w.double().permute(0, 2, 3, 1).reshape(64, 9 * 96)  # k = tap * ci + c
    got = unpack_x2(fwd, 64, 9 * 96)
    floor = lambda r: r.abs().amax(1, keepdim=True) * 2.0 ** -37  # noqa: E731  fp16 subnormal floor
    assert ((got - ref_f).abs() <= ref_f.abs() * 2.0 ** -21 + floor(ref_f)).all()
    us = fwd[64 * 9 * 96:].cpu()
    assert torch.all(torch.log2(us) == torch.round(torch.log2(us)))  # powers of two
    wt = w.flip(2, 3).transpose(0, 1)  # the data-gradient conv's kernel [ci][co][3][3]
    ref_d = wt.double().permute(0, 2, 3, 1).reshape(96, 9 * 64)
    got_d = unpack_x2(dg, 96, 9 * 64)
    assert ((got_d - ref_d).abs() <= ref_d.abs() * 2.0 ** -21 + floor(ref_d)).all()


def test_x2_eligibility():
    ok = lambda *a: K.query("selunet_conv3x3_x2_ok", *a)  # noqa: E731
    assert ok(32, 32, 64, 64, 64) == 1
    assert ok(32, 32, 32, 32, 64) == 0    # one channel chunk
    assert ok(8, 8, 64, 64, 64) == 0      # below the 16x16 halo tile
    assert ok(32, 31, 64, 64, 64) == 1    # odd widths are fine (direct form)
    assert ok(32, 32, 64, 64, 96) == 0


def word(v):
    return torch.tensor([float(v)], device=DEV)


@pytest.mark.parametrize("cin0,cin1,cout,n,h,w,xform", [
    (64, 0, 64, 2, 16, 16, True),
    (64, 64, 128, 1, 16, 48, True),     # two sources (torch.cat), BN = 128
    (128, 0, 256, 2, 20, 24, True),     # partial edge tiles
    (256, 0, 128, 2, 32, 32, False),
    (128, 128, 64, 1, 32, 16, True),    # two sources, BN = 64
    (64, 0, 128, 1, 18, 35, True),      # partial tiles in both directions, odd width
    (64, 0, 64, 2, 64, 48, True),       # 64 columns (two workgroups per CU): several tiles per workgroup
    (64, 64, 64, 1, 40, 72, True),      # 64 columns, two sources, partial tiles, four chunks
])
@pytest.mark.parametrize("wgs", [0, 3])
@pytest.mark.parametrize("x2d_mode,tq", [(1, 0), (0, 0), (0, 1), (0, 2)])
def test_x2_fwd_stats(cin0, cin1, cout, n, h, w, xform, wgs, x2d_mode, tq, halo_wgs, x2d, tile_queue):
    halo_wgs(wgs)
    x2d(x2d_mode)
    tile_queue(tq)
    x2_fwd_stats_case(cin0, cin1, cout, n, h, w, xform)


@pytest.mark.parametrize("cin0,cin1,cout,n,h,w", [(64, 0, 64, 2, 16, 16), (64, 64, 128, 1, 16, 48)])
@pytest.mark.parametrize("x2d_mode,tq", [(1, 0), (0, 0), (0, 1), (0, 2)])
@pytest.mark.parametrize("slack", SLACKS)
def test_x2_fwd_stats_loose_words(cin0, cin1, cout, n, h, w, x2d_mode, tq, slack, x2d, tile_queue):
    x2d(x2d_mode)
    tile_queue(tq)
    x2_fwd_stats_case(cin0, cin1, cout, n, h, w, True, slack=slack)


@pytest.mark.parametrize("x2d_mode,tq", [(1, 0), (0, 0), (0, 1), (0, 2)])
def test_x2_fwd_zero_second_source(x2d_mode, tq, x2d, tile_queue):
    """A two-source forward whose second source is all zeros with amax1 = 0 (x2_scale's amax = 0 branch)."""
    x2d(x2d_mode)
    tile_queue(tq)
    x2_fwd_stats_case(64, 64, 64, 1, 16, 48, True, zero_src1=True)
    x2_fwd_stats_case(64, 64, 128, 1, 16, 48, True, zero_src1=True)


def x2_fwd_stats_case(cin0, cin1, cout, n, h, w, xform, signed=False, slack=1.0, zero_src1=False):
    x0 = gen(n, cin0, h, w, seed=1)
    x1 = gen(n, cin1, h, w, seed=2) * 1e-3 if cin1 else None  # sources of different ranges
    wt = gen(cout, cin0 + cin1, 3, 3, seed=3, scale=0.05)
    s0, t0 = bn_fold(cin0, 10, signed)
    a0 = torch.relu(x0 * s0.view(1, -1, 1, 1) + t0.view(1, -1, 1, 1)) if xform else x0
    a = a0
    if cin1:
        s1, t1 = bn_fold(cin1, 12, signed)
        if zero_src1:  # relu(0 * s + t) = 0 everywhere
            x1, t1 = torch.zeros_like(x1), -t1.abs()
        a1 = torch.relu(x1 * s1.view(1, -1, 1, 1) + t1.view(1, -1, 1, 1))
        assert not zero_src1 or float(a1.abs().max()) == 0.0
        a = torch.cat((a0, a1), 1)
    if signed:
        # (the second source's values are 1e-3 of its shift: its ReLU follows the shift's sign alone)
        check_signed_inputs(torch.cat((s0, s1)) if cin1 else s0, a)
    ref = F.conv2d(a.double(), wt.double(), padding=1)
    assert K.query("selunet_conv3x3_x2_ok", h, w, cin0 + cin1, cin0, cout) == 1
    u, _ = pack_x2(wt, dgrad=False)
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    keep = [d(nhwc(x0)), d(s0), d(t0)]  # K.source holds raw pointers: the tensors must stay alive
    srcs = [K.source(keep[0], cin0, keep[1] if xform else None, keep[2] if xform else None)]
    am0, am1 = word(a0.abs().max() * 1.5 * slack), None
    if cin1:
        keep += [d(nhwc(x1)), d(s1), d(t1)]
        srcs.append(K.source(keep[3], cin1, keep[4], keep[5]))
        am1 = word(a1.abs().max() * slack)
    M = n * h * w
    y = torch.empty(M, cout, device=DEV)
    g = K.gather(n, h, w, 9, *srcs)
    rows = K.query("selunet_conv3x3_x2_stats_rows", g, cout)
    stats = torch.empty(rows, 2, cout, device=DEV)
    ep = K.Epilogue(K.ptr(y), None, None, K.ptr(stats), K.EP_PLAIN, 0)
    K.call("selunet_conv3x3_x2", g, K.ptr(u), cout, ep, K.ptr(am0), K.ptr(am1), K.stream_ptr())
    torch.cuda.synchronize()
    assert rel(nchw(y.cpu(), n, h, w), ref) < TOL
    st = stats.cpu().double().sum(0)
    r = ref.permute(1, 0, 2, 3).reshape(cout, -1)
    assert rel(st[0], r.sum(1)) < TOL and rel(st[1], (r * r).sum(1)) < TOL


@pytest.mark.parametrize("cin,cout,split,h,w", [(64, 64, 0, 32, 32), (128, 64, 64, 32, 32),
                                                (256, 128, 128, 16, 48), (128, 256, 0, 20, 24),
                                                (512, 256, 256, 16, 16), (64, 64, 0, 64, 48),
                                                (64, 128, 0, 48, 40)])
@pytest.mark.parametrize("wgs", [0, 3])
@pytest.mark.parametrize("x2d_mode,tq", [(1, 0), (0, 0), (0, 1), (0, 2)])
def test_x2_dgrad(cin, cout, split, h, w, wgs, x2d_mode, tq, halo_wgs, x2d, tile_queue):
    """Gradient-sized operands (1e-9 scale): the range word rescales them into the fp16 range."""
    halo_wgs(wgs)
    x2d(x2d_mode)
    tile_queue(tq)
    x2_dgrad_case(cin, cout, split, h, w)


@pytest.mark.parametrize("cin,cout,split,h,w", [(64, 64, 0, 32, 32), (128, 64, 64, 32, 32)])
@pytest.mark.parametrize("x2d_mode,tq", [(1, 0), (0, 0), (0, 1), (0, 2)])
@pytest.mark.parametrize("slack", SLACKS)
def test_x2_dgrad_loose_words(cin, cout, split, h, w, x2d_mode, tq, slack, x2d, tile_queue):
    x2d(x2d_mode)
    tile_queue(tq)
    x2_dgrad_case(cin, cout, split, h, w, slack=slack)


@pytest.mark.parametrize("x2d_mode,tq", [(1, 0), (0, 0), (0, 1), (0, 2)])
def test_x2_dgrad_zero_operand(x2d_mode, tq, x2d, tile_queue):
    """dy = 0 with range word 0.0 (x2_scale's amax = 0 branch): the output is exactly zero and finite, the output
    word is 0 and the BN-backward sums are (0, 0, sum xhat) (x2_dgrad_case's checks at a zero reference)."""
    x2d(x2d_mode)
    tile_queue(tq)
    x2_dgrad_case(64, 64, 0, 32, 32, zero=True)
    x2_dgrad_case(128, 64, 0, 32, 32, zero=True)  # 128 columns


def x2_dgrad_case(cin, cout, split, h, w, signed=False, slack=1.0, zero=False):
    n = 2
    wt = gen(cout, cin, 3, 3, seed=6, scale=0.05)
    dy = gen(n, cout, h, w, seed=7) * (0.0 if zero else 1e-9)
    x = gen(n, cin, h, w, seed=8).double().requires_grad_()
    (ref,) = torch.autograd.grad(F.conv2d(x, wt.double(), padding=1), x, dy.double())
    _, dg = pack_x2(wt)
    M = n * h * w
    dyd = nhwc(dy).to(DEV)  # kept alive: K.source holds the raw pointer
    am = word(dy.abs().max() * slack)
    g = K.gather(n, h, w, 9, K.source(dyd, cout))
    rows = K.query("selunet_conv3x3_x2_stats_rows", g, cin)
    if split:
        d0 = torch.empty(M, split, device=DEV)
        d1 = torch.empty(M, cin - split, device=DEV)
        colsum = torch.empty(rows, split, device=DEV)
        ep = K.Epilogue(K.ptr(d0), K.ptr(d1), None, None, K.EP_SPLIT, split, K.ptr(colsum))
        word_out = torch.zeros(1, device=DEV)
        ep.amax = K.ptr(word_out)
        K.call("selunet_conv3x3_x2", g, K.ptr(dg), cin, ep, K.ptr(am), None, K.stream_ptr())
        got = torch.cat((nchw(d0.cpu(), n, h, w), nchw(d1.cpu(), n, h, w)), 1)
        assert rel(colsum.double().sum(0).cpu(), d0.double().sum(0).cpu()) < 1e-6
        # the range word: the exact max |stored value| over both outputs (every kernel variant)
        assert word_out.item() == max(d0.abs().max().item(), d1.abs().max().item())
    else:
        dx = torch.empty(M, cin, device=DEV)
        yprev = gen(M, cin, seed=42).to(DEV)
        sc, sh, mean, invstd = bnb_operands(cin, 43, signed)
        if signed:
            check_signed_inputs(sc, torch.relu(yprev * sc + sh))
        slab = torch.empty(rows, 3, cin, device=DEV)
        ep = K.Epilogue(K.ptr(dx), None, None, None, K.EP_PLAIN, 0)
        ep.bnb = K.BnBwdStats(K.ptr(yprev), K.ptr(sc), K.ptr(sh), K.ptr(mean), K.ptr(invstd), K.ptr(slab))
        word_out = torch.full((1,), 0.0, device=DEV)
        ep.amax = K.ptr(word_out)
        K.call("selunet_conv3x3_x2", g, K.ptr(dg), cin, ep, K.ptr(am), None, K.stream_ptr())
        got = nchw(dx.cpu(), n, h, w)
        check_bnb_sums(slab, dx, yprev, sc, sh, mean, invstd)
        assert word_out.item() == dx.abs().max().item()  # the range word: the exact max |stored value|
        if zero:
            assert word_out.item() == 0.0 and bool((dx == 0).all())
            s3 = slab.double().sum(0)
            assert bool((s3[:2] == 0).all())
    torch.cuda.synchronize()
    if zero:
        assert bool((got == 0).all())
    else:
        assert rel(got, ref) < TOL


@pytest.mark.parametrize("cin,cout,n,h,w", [(128, 128, 2, 40, 48), (256, 64, 1, 32, 80)])
def test_x2_tile_queue_is_schedule_independent(cin, cout, n, h, w, halo_wgs, x2d, tile_queue):
    """SELUNET_OPT_TILE_QUEUE: pixel tiles taken from a ticket counter, statistics flushed per tile into slab
    row = tile index, so the outputs, the BN-backward sums and the range word are bit-identical whichever
    workgroup ran a tile — here under three workgroup counts (and so three assignments) and two repeats
    (the counters reset themselves between launches)."""
    x2d(0)
    tile_queue(1)
    wt = gen(cout, cin, 3, 3, seed=6, scale=0.05)
    dy = nhwc(gen(n, cout, h, w, seed=7) * 1e-6).to(DEV)
    _, dg = pack_x2(wt)
    M = n * h * w
    am = word(dy.abs().max())
    g = K.gather(n, h, w, 9, K.source(dy, cout))
    rows = K.query("selunet_conv3x3_x2_stats_rows", g, cin)
    assert rows == n * ((h + 15) // 16) * ((w + 15) // 16)  # one slab row per pixel tile
    yprev = gen(M, cin, seed=42).to(DEV)
    sc, sh = (gen(cin, seed=43).abs() + 0.5).to(DEV), (gen(cin, seed=44) * 0.3).to(DEV)
    mean, invstd = (gen(cin, seed=45) * 0.1).to(DEV), (gen(cin, seed=46).abs() + 0.5).to(DEV)
    outs = []
    for wgs in (0, 3, 7, 0):
        halo_wgs(wgs)
        dx = torch.empty(M, cin, device=DEV)
        slab = torch.full((rows, 3, cin), float("nan"), device=DEV)
        amax = torch.zeros(1, device=DEV)
        ep = K.Epilogue(K.ptr(dx), None, None, None, K.EP_PLAIN, 0)
        ep.bnb = K.BnBwdStats(K.ptr(yprev), K.ptr(sc), K.ptr(sh), K.ptr(mean), K.ptr(invstd), K.ptr(slab))
        ep.amax = K.ptr(amax)
        K.call("selunet_conv3x3_x2", g, K.ptr(dg), cin, ep, K.ptr(am), None, K.stream_ptr())
        torch.cuda.synchronize()
        outs.append((dx.cpu(), slab.cpu(), amax.item()))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) and o[2] == outs[0][2]
    assert not torch.isnan(outs[0][1]).any()
    # the range word is the exact max |stored value| (round 6: the tile-queue path left it 0)
    assert outs[0][2] == outs[0][0].abs().max().item() > 0
    check_bnb_sums(slab, dx, yprev, sc, sh, mean, invstd)


def test_tile_queue_training_matches_static():
    """60 training steps at 16 x 256^2 (the 8-GPU shard) with SELUNET_OPT_TILE_QUEUE against the static walk: the
    per-step losses agree to split-fp16 rounding. (Round 6 found the tile-queue path's range word left at 0: the
    consumer scaled by 2^14 and its fp16 split overflowed once values passed 4 — after ~45 steps the loss jumped
    from 0.41 to 1.21, while every single-launch test passed.)"""
    from selectivenet_for_semantic_segmentation_binary_amd.synthetic import make_batch
    import selectivenet_for_semantic_segmentation_binary_amd as S
    from tests.test_gpu_model import build
    x, lab = make_batch(16, 256, seed=0)
    xt, lt = torch.tensor(x, device=DEV), torch.tensor(lab, device=DEV)
    runs = []
    for tq in (0, 1, 2, 3):  # static, the convolutions' tile queue, the weight gradients', both
        prev = K.set_option("TILE_QUEUE", tq)
        try:
            net = build(True)
            opt = S.Adam(net.parameters(), lr=1e-3)
            la = S.BCEWithLogitsLoss()
            losses = []
            for _ in range(60):
                o, sel, a = net(xt)
                loss = la(a, lt) + S.calc_selective_risk_image_b(o, sel, target=lt, lamb=2)[0]
                opt.zero_grad()
                loss.backward()
                opt.step()
                losses.append(float(loss.item()))
            runs.append(np.array(losses))
        finally:
            K.set_option("TILE_QUEUE", prev)
    # Rounding-level differences grow along a training trajectory: the deterministic conv queue (1) ends 60 steps
    # 7.8e-4 from the static walk, the weight-gradient queues (2, 3), whose summation order changes run to run,
    # 1.1e-3 in one run (r06). The bound is 5e-3 — the failure it guards against moved the loss by a factor 3.
    for k in (1, 2, 3):
        dev = np.abs(runs[k] - runs[0]) / np.abs(runs[0])
        print(f"tile queue {k} vs static over 60 steps: max relative loss deviation {dev.max():.2e}")
        assert dev.max() < 5e-3, (k, dev.argmax(), runs[0][dev.argmax()], runs[k][dev.argmax()])


def test_x2_rejects():
    n, h, w, c = 1, 8, 8, 64
    x = torch.zeros(n * h * w, c, device=DEV)
    u = torch.zeros(64 * 9 * c + 64, device=DEV)
    y = torch.empty(n * h * w, 64, device=DEV)
    am = word(1.0)
    ep = K.Epilogue(K.ptr(y), None, None, None, K.EP_PLAIN, 0)
    with pytest.raises(K.SelunetError):  # below the halo tile
        K.call("selunet_conv3x3_x2", K.gather(n, h, w, 9, K.source(x, c)), K.ptr(u), 64, ep, K.ptr(am), None,
               K.stream_ptr())
    h = w = 16
    x = torch.zeros(n * h * w, c, device=DEV)
    y = torch.empty(n * h * w, 64, device=DEV)
    ep = K.Epilogue(K.ptr(y), None, None, None, K.EP_PLAIN, 0)
    with pytest.raises(K.SelunetError):  # no range word
        K.call("selunet_conv3x3_x2", K.gather(n, h, w, 9, K.source(x, c)), K.ptr(u), 64, ep, None, None,
               K.stream_ptr())


def test_act_bound():
    """Samuelson: |xhat| <= sqrt(count - 1) under batch statistics, so the word bounds relu(bn(y))."""
    act_bound_case(False)


def test_act_bound_signed():
    """The largest |gamma| and the largest |beta| are both negative (a dropped absolute value would lose
    them), with signed_gamma's negative group and exact zeros among the rest."""
    act_bound_case(True)


def act_bound_case(signed):
    c, count = 96, 5000
    gamma, beta = gen(c, seed=1), gen(c, seed=2)
    if signed:
        gamma = signed_gamma(c, 1)
        gamma[2], beta[11] = -1.5 * gamma.abs().max(), -1.5 * beta.abs().max()
        assert float((gamma < 0).float().mean()) >= 0.25
        assert gamma.abs().max() == -gamma.min() and beta.abs().max() == -beta.min()
    gamma, beta = gamma.to(DEV), beta.to(DEV)
    out = torch.empty(1, device=DEV)
    K.call("selunet_act_bound", K.ptr(gamma), K.ptr(beta), c, count, K.ptr(out), K.stream_ptr())
    want = gamma.abs().max().item() * count ** 0.5 + beta.abs().max().item()
    assert abs(out.item() - want) <= 2e-4 * want
    # an adversarial batch: one outlier per channel reaches the bound's sqrt(count - 1) * sigma
    y = torch.zeros(count, c, dtype=torch.float64)
    y[0] = 1.0
    xhat = (y - y.mean(0)) / y.std(0, unbiased=False)
    a = (xhat * gamma.cpu().double() + beta.cpu().double()).abs().max().item()
    assert a <= out.item()


def test_bn_bwd_apply_amax_and_epilogue_amax():
    m, c = 4096, 64
    dz, y = gen(m, c, seed=1).to(DEV), gen(m, c, seed=2).to(DEV)
    sc, sh = (gen(c, seed=3).abs() + 0.5).to(DEV), gen(c, seed=4).to(DEV)
    mean, invstd = (gen(c, seed=5) * 0.1).to(DEV), (gen(c, seed=6).abs() + 0.5).to(DEV)
    coef = gen(3, c, seed=7).to(DEV) * 1e-3
    dy, dy2 = torch.empty(m, c, device=DEV), torch.empty(m, c, device=DEV)
    am = torch.zeros(1, device=DEV)
    args = [K.ptr(t) for t in (dz, y)] + [m, c] + [K.ptr(t) for t in (sc, sh, mean, invstd, coef)]
    K.call("selunet_bn_bwd_apply", *args, K.ptr(dy), K.F32, K.stream_ptr())
    K.call("selunet_bn_bwd_apply_amax", *args, K.ptr(dy2), K.ptr(am), K.F32, K.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(dy, dy2) and am.item() == dy.abs().max().item()
    # ConvTranspose2d forward (SCATTER2X) with the output range word
    n, h, w, ci, co = 2, 8, 8, 64, 32
    x = gen(n * h * w, ci, seed=8).to(DEV)
    wp = gen(4 * co, ci, seed=9, scale=0.1).to(DEV)
    bias = gen(co, seed=10).to(DEV)
    up = torch.empty(n * 4 * h * w, co, device=DEV)
    am2 = torch.zeros(1, device=DEV)
    ep = K.Epilogue(K.ptr(up), None, K.ptr(bias), None, K.EP_SCATTER2X, 0)
    ep.amax = K.ptr(am2)
    K.call("selunet_gemm_gather", K.gather(n, h, w, 1, K.source(x, ci)), K.ptr(wp), 4 * co, ci, ep, K.F32,
           K.stream_ptr())
    torch.cuda.synchronize()
    assert am2.item() == up.abs().max().item()


@pytest.mark.parametrize("cin0,cin1,cout,xform,n,h,w", [
    (64, 0, 64, True, 2, 16, 16),
    (64, 64, 128, True, 2, 16, 16),     # two sources (torch.cat) of different ranges, BN+ReLU staging
    (128, 0, 256, False, 1, 20, 36),    # ragged 8x8 tiles in both directions
    (256, 0, 64, True, 3, 12, 18),      # ragged rows, odd tile counts, BI = 64 (two tap groups)
    (128, 0, 128, True, 2, 9, 17),      # odd sizes
])
def test_x2_wgrad(cin0, cin1, cout, xform, n, h, w):
    """Split-fp16 weight gradient (conv3x3_wgrad_x2_kernel + the fixed-order split reduction into the
    Conv2d layout) against torch's conv2d weight gradient in fp64; gradient-sized dY (1e-9)."""
    x2_wgrad_case(cin0, cin1, cout, xform, n, h, w)


@pytest.mark.parametrize("cin0,cin1,cout", [(64, 0, 64), (64, 64, 128)])
@pytest.mark.parametrize("slack", SLACKS)
def test_x2_wgrad_loose_words(cin0, cin1, cout, slack):
    x2_wgrad_case(cin0, cin1, cout, True, 2, 16, 16, slack=slack)


def x2_wgrad_case(cin0, cin1, cout, xform, n, h, w, signed=False, slack=1.0):
    x0 = gen(n, cin0, h, w, seed=9)
    s0, t0 = bn_fold(cin0, 20, signed)
    a0 = torch.relu(x0 * s0.view(1, -1, 1, 1) + t0.view(1, -1, 1, 1)) if xform else x0
    a = a0
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    keep = [d(nhwc(x0)), d(s0), d(t0)]
    srcs = [K.source(keep[0], cin0, keep[1] if xform else None, keep[2] if xform else None)]
    am1 = None
    if cin1:
        x1 = gen(n, cin1, h, w, seed=10) * 1e-3
        s1, t1 = bn_fold(cin1, 22, signed)
        a1 = torch.relu(x1 * s1.view(1, -1, 1, 1) + t1.view(1, -1, 1, 1))
        a = torch.cat((a0, a1), 1)
        keep += [d(nhwc(x1)), d(s1), d(t1)]
        srcs.append(K.source(keep[3], cin1, keep[4], keep[5]))
        am1 = word(a1.abs().max() * slack)
    if signed:
        check_signed_inputs(torch.cat((s0, s1)) if cin1 else s0, a)
    am0 = word(a0.abs().max() * slack)
    cin = cin0 + cin1
    wt = gen(cout, cin, 3, 3, seed=11, scale=0.05).double().requires_grad_()
    dy = gen(n, cout, h, w, seed=12) * 1e-9
    (ref,) = torch.autograd.grad(F.conv2d(a.double(), wt, padding=1), wt, dy.double())
    dyd = d(nhwc(dy))
    amp = word(dy.abs().max() * slack)
    gp, gq = K.gather(n, h, w, 1, K.source(dyd, cout)), K.gather(n, h, w, 9, *srcs)
    wsb = K.query("selunet_conv3x3_wgrad_x2_ws_bytes", gp, gq)
    assert wsb > 0
    ws = torch.empty(wsb // 4, device=DEV)
    outs = []
    for _ in range(2):
        out = torch.full((cout, cin, 3, 3), float("nan"), device=DEV)
        K.call("selunet_conv3x3_wgrad_x2", gp, gq, K.ptr(ws), wsb, K.ptr(out), K.ptr(amp), K.ptr(am0), K.ptr(am1),
               K.stream_ptr())
        outs.append(out)
    torch.cuda.synchronize()
    assert rel(outs[0].cpu(), ref) < TOL
    assert torch.equal(outs[0], outs[1])  # fixed-order reduction: bit-reproducible


@pytest.mark.parametrize("cin,cout,n,h,w", [(128, 256, 2, 20, 36), (256, 64, 3, 12, 18), (512, 512, 2, 16, 16)])
def test_x2_wgrad_tile_queue(cin, cout, n, h, w):
    """SELUNET_OPT_TILE_QUEUE bit 1 (= 2): the weight gradient's (co tile, ci chunk) groups take their pixel tiles from
    ticket counters. Every tile is summed exactly once whatever the assignment: against the fp64 weight gradient
    at the split-fp16 tolerance and against the static walk to rounding, under three workgroup targets (one, a
    few and many workgroups per group) and repeated launches (the counters reset themselves)."""
    x = gen(n, cin, h, w, seed=31)
    s0, t0 = bn_fold(cin, 32)
    a = torch.relu(x * s0.view(1, -1, 1, 1) + t0.view(1, -1, 1, 1))
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    keep = [d(nhwc(x)), d(s0), d(t0)]
    gq = K.gather(n, h, w, 9, K.source(keep[0], cin, keep[1], keep[2]))
    wt = gen(cout, cin, 3, 3, seed=33, scale=0.05).double().requires_grad_()
    dy = gen(n, cout, h, w, seed=34) * 1e-9
    (ref,) = torch.autograd.grad(F.conv2d(a.double(), wt, padding=1), wt, dy.double())
    dyd = d(nhwc(dy))
    amp, am0 = word(dy.abs().max()), word(a.abs().max())
    gp = K.gather(n, h, w, 1, K.source(dyd, cout))
    outs = {}
    prev_tq = K.set_option("TILE_QUEUE", 0)
    prev_wgs = K.set_option("X2_WGRAD_WGS", 256)
    try:
        for tq, wgs in [(0, 256), (2, 256), (2, 64), (2, 2048), (2, 256)]:
            K.set_option("TILE_QUEUE", tq)
            K.set_option("X2_WGRAD_WGS", wgs)
            wsb = K.query("selunet_conv3x3_wgrad_x2_ws_bytes", gp, gq)
            ws = torch.empty(wsb // 4, device=DEV)
            out = torch.full((cout, cin, 3, 3), float("nan"), device=DEV)
            K.call("selunet_conv3x3_wgrad_x2", gp, gq, K.ptr(ws), wsb, K.ptr(out), K.ptr(amp), K.ptr(am0), None,
                   K.stream_ptr())
            torch.cuda.synchronize()
            outs.setdefault((tq, wgs), []).append(out.cpu())
    finally:
        K.set_option("TILE_QUEUE", prev_tq)
        K.set_option("X2_WGRAD_WGS", prev_wgs)
    static = outs[(0, 256)][0]
    assert rel(static, ref) < TOL
    for key, lst in outs.items():
        for o in lst:
            assert not torch.isnan(o).any(), key
            assert rel(o, ref) < TOL, key
            assert rel(o, static.double()) < 1e-6, key


def pack_convT_x2(w):
    """Split-fp16 ConvTranspose2d operands of w [ci][co][2][2]: fwd [4co][ci] + 4co, dgrad [ci][4co] + ci."""
    ci, co = w.shape[:2]
    wd = w.to(DEV).contiguous()
    fwd = torch.empty(4 * co * ci + 4 * co, device=DEV)
    dg = torch.empty(ci * 4 * co + ci, device=DEV)
    pl = K.PackList()
    pl.d[0] = K.PackDesc(K.ptr(wd), K.ptr(fwd), K.ptr(dg), K.PACK_CONVT_X2, co, ci, ci, 0)
    pl.n = 1
    K.call("selunet_pack_weights", pl, K.F32, K.stream_ptr())
    return fwd, dg


@pytest.mark.parametrize("cin,cout", [(512, 256), (128, 64)])
@pytest.mark.parametrize("gwgs", [-1, 0, 3])
def test_x2_convT_fwd_dgrad(cin, cout, gwgs, gather_wgs):
    """ConvTranspose2d forward (SCATTER2X + bias, output range word) and data gradient (taps=4, with the
    BN-backward sums epilogue) through selunet_gemm_gather_x2, against torch in fp64."""
    gather_wgs(gwgs)
    x2_convT_fwd_dgrad_case(cin, cout)


@pytest.mark.parametrize("slack", SLACKS)
def test_x2_convT_fwd_dgrad_loose_words(slack):
    x2_convT_fwd_dgrad_case(128, 64, slack=slack)


def x2_convT_fwd_dgrad_case(cin, cout, signed=False, slack=1.0):
    n, h, w = 2, 13, 18
    x = gen(n, cin, h, w, seed=13)
    s, t = bn_fold(cin, 30, signed)
    a = torch.relu(x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)).double().requires_grad_()
    if signed:
        check_signed_inputs(s, a.detach())
    wt = gen(cin, cout, 2, 2, seed=14, scale=0.05).double()
    b = gen(cout, seed=15).double()
    y = F.conv_transpose2d(a, wt, b, stride=2)
    dy = gen(*y.shape, seed=16) * 1e-8
    (ga,) = torch.autograd.grad(y, (a,), dy.double())
    fwd, dg = pack_convT_x2(wt.float())
    torch.cuda.synchronize()
    ref_f = wt.permute(2, 3, 1, 0).reshape(4 * cout, cin)  # row (a*2+b)*co + o, k = c
    assert rel(unpack_x2(fwd, 4 * cout, cin), ref_f) < 1e-6
    d = lambda t_: t_.to(DEV).contiguous()  # noqa: E731
    xd, sd, td, bd = d(nhwc(x)), d(s), d(t), d(b.float())
    up = torch.empty(n * 2 * h * 2 * w, cout, device=DEV)
    amu = torch.zeros(1, device=DEV)
    ep = K.Epilogue(K.ptr(up), None, K.ptr(bd), None, K.EP_SCATTER2X, 0)
    ep.amax = K.ptr(amu)
    am = word(a.detach().abs().max() * slack)
    K.call("selunet_gemm_gather_x2", K.gather(n, h, w, 1, K.source(xd, cin, sd, td)), K.ptr(fwd), 4 * cout, cin, ep,
           K.ptr(am), None, K.stream_ptr())
    torch.cuda.synchronize()
    assert rel(nchw(up.cpu(), n, 2 * h, 2 * w), y) < TOL
    assert amu.item() == up.abs().max().item()
    dud = d(nhwc(dy))
    amd = word(dy.abs().max() * slack)
    da = torch.empty(n * h * w, cin, device=DEV)
    M = n * h * w
    yprev = gen(M, cin, seed=42).to(DEV)
    sc, sh, mean, invstd = bnb_operands(cin, 43, signed)
    if signed:
        check_signed_inputs(sc, torch.relu(yprev * sc + sh))
    g4 = K.gather(n, h, w, 4, K.source(dud, cout))
    rows = K.query("selunet_gemm_gather_x2_stats_rows", g4, cin)
    slab = torch.empty(rows, 3, cin, device=DEV)
    ep = K.Epilogue(K.ptr(da), None, None, None, K.EP_PLAIN, 0)
    ep.bnb = K.BnBwdStats(K.ptr(yprev), K.ptr(sc), K.ptr(sh), K.ptr(mean), K.ptr(invstd), K.ptr(slab))
    K.call("selunet_gemm_gather_x2", g4, K.ptr(dg), cin, 4 * cout, ep, K.ptr(amd), None, K.stream_ptr())
    torch.cuda.synchronize()
    assert rel(nchw(da.cpu(), n, h, w), ga) < TOL
    check_bnb_sums(slab, da, yprev, sc, sh, mean, invstd)


@pytest.mark.parametrize("cin,cout,n,h,w", [(128, 64, 2, 9, 64), (256, 128, 2, 9, 64), (256, 128, 1, 5, 32),
                                             (128, 64, 4, 72, 512)])
def test_x2_convT_dgrad_resident(cin, cout, n, h, w):
    """ConvTranspose2d data gradient on the resident-weight kernel (convt_dgrad_x2_kernel: K = 4*cout of
    256 / 512, w % 32 == 0; partial last tiles, and several tiles per workgroup at 4x72x512) against torch
    in fp64, with the BN-backward sums checked against the sums of its own output."""
    x = gen(n, cin, h, w, seed=23)
    a = x.double().requires_grad_()
    wt = gen(cin, cout, 2, 2, seed=24, scale=0.05).double()
    y = F.conv_transpose2d(a, wt, None, stride=2)
    dy = gen(*y.shape, seed=25) * 1e-3
    (ga,) = torch.autograd.grad(y, (a,), dy.double())
    _, dg = pack_convT_x2(wt.float())
    d = lambda t_: t_.to(DEV).contiguous()  # noqa: E731
    dud = d(nhwc(dy))
    amd = word(dy.abs().max())
    M = n * h * w
    da = torch.empty(M, cin, device=DEV)
    yprev = gen(M, cin, seed=47).to(DEV)
    sc, sh = (gen(cin, seed=48).abs() + 0.5).to(DEV), (gen(cin, seed=49) * 0.3).to(DEV)
    mean, invstd = (gen(cin, seed=50) * 0.1).to(DEV), (gen(cin, seed=51).abs() + 0.5).to(DEV)
    g4 = K.gather(n, h, w, 4, K.source(dud, cout))
    rows = K.query("selunet_gemm_gather_x2_stats_rows", g4, cin)
    ntb = 128 if cout == 64 else 64
    tile = 8 * (8 // (ntb // 32)) * 32
    assert rows == min(-(-M // tile), 256 // (cin // ntb))  # the resident-weight kernel's workgroup rows
    slab = torch.full((rows, 3, cin), float("nan"), device=DEV)
    amo = torch.zeros(1, device=DEV)
    ep = K.Epilogue(K.ptr(da), None, None, None, K.EP_PLAIN, 0)
    ep.bnb = K.BnBwdStats(K.ptr(yprev), K.ptr(sc), K.ptr(sh), K.ptr(mean), K.ptr(invstd), K.ptr(slab))
    ep.amax = K.ptr(amo)
    K.call("selunet_gemm_gather_x2", g4, K.ptr(dg), cin, 4 * cout, ep, K.ptr(amd), None, K.stream_ptr())
    torch.cuda.synchronize()
    assert rel(nchw(da.cpu(), n, h, w), ga) < TOL
    assert amo.item() == da.abs().max().item()
    y64, g64 = yprev.double(), da.double() * (yprev.double() * sc.double() + sh.double() > 0).double()
    xh = (y64 - mean.double()) * invstd.double()
    terms = [g64, g64 * xh, xh]
    got = slab.double().sum(0)
    for k in range(3):
        err = (got[k] - terms[k].sum(0)).abs() / (terms[k].abs().sum(0) + 1e-30)
        assert float(err.max()) < 1e-6, (k, float(err.max()))


@pytest.fixture
def convt_ring():
    """Set SELUNET_OPT_CONVT_RING for one test (0: the resident-weight / staged kernels)."""
    prev = []

    def setter(mode):
        prev.append(K.set_option("CONVT_RING", mode))
    yield setter
    for v in prev[:1]:
        K.set_option("CONVT_RING", v)


def _convT_x2_pair(cin, cout, n, h, w, seed, signed=False, slack=1.0):
    """Forward (+ bias, range word) and data gradient (+ BN-backward sums, range word) of one
    ConvTranspose2d through selunet_gemm_gather_x2 with whatever kernels the options select."""
    x = gen(n, cin, h, w, seed=seed)
    s, t = bn_fold(cin, seed + 1, signed)
    wt = gen(cin, cout, 2, 2, seed=seed + 2, scale=0.05)
    b = gen(cout, seed=seed + 3)
    dy = gen(n, cout, 2 * h, 2 * w, seed=seed + 4) * 1e-3
    fwd, dg = pack_convT_x2(wt)
    d = lambda t_: t_.to(DEV).contiguous()  # noqa: E731
    xd, sd, td, bd = d(nhwc(x)), d(s), d(t), d(b)
    M = n * h * w
    up = torch.empty(M * 4, cout, device=DEV)
    amu = torch.zeros(1, device=DEV)
    ep = K.Epilogue(K.ptr(up), None, K.ptr(bd), None, K.EP_SCATTER2X, 0)
    ep.amax = K.ptr(amu)
    am = word(torch.relu(x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)).abs().max() * slack)
    K.call("selunet_gemm_gather_x2", K.gather(n, h, w, 1, K.source(xd, cin, sd, td)), K.ptr(fwd), 4 * cout, cin, ep,
           K.ptr(am), None, K.stream_ptr())
    dud = d(nhwc(dy))
    amd = word(dy.abs().max() * slack)
    da = torch.empty(M, cin, device=DEV)
    yprev = gen(M, cin, seed=seed + 5).to(DEV)
    sc, sh, mean, invstd = bnb_operands(cin, seed + 6, signed)
    g4 = K.gather(n, h, w, 4, K.source(dud, cout))
    rows = K.query("selunet_gemm_gather_x2_stats_rows", g4, cin)
    slab = torch.full((rows, 3, cin), float("nan"), device=DEV)
    amo = torch.zeros(1, device=DEV)
    ep = K.Epilogue(K.ptr(da), None, None, None, K.EP_PLAIN, 0)
    ep.bnb = K.BnBwdStats(K.ptr(yprev), K.ptr(sc), K.ptr(sh), K.ptr(mean), K.ptr(invstd), K.ptr(slab))
    ep.amax = K.ptr(amo)
    K.call("selunet_gemm_gather_x2", g4, K.ptr(dg), cin, 4 * cout, ep, K.ptr(amd), None, K.stream_ptr())
    torch.cuda.synchronize()
    return dict(x=x, s=s, t=t, wt=wt, b=b, dy=dy, up=up, amu=amu, da=da, amo=amo, slab=slab, rows=rows,
                yprev=yprev, sc=sc, sh=sh, mean=mean, invstd=invstd)


@pytest.mark.parametrize("cin,cout,n,h,w", [
    (512, 256, 2, 32, 32),    # unpool3 at a 2-image shard: forward K 512 / N 1024, data gradient K 1024 / N 512
    (256, 128, 1, 64, 64),    # unpool2: forward K 256 / N 512, data gradient K 512 / N 256
    (512, 256, 1, 16, 32),    # one row tile: more column blocks than row tiles
])
def test_x2_convT_ring(cin, cout, n, h, w, convt_ring):
    """The LDS-DMA ring kernel (convt_ring_x2_kernel, ConvTranspose2d forward and data gradient with
    K >= 256 on 256-column blocks) against torch in fp64: output, output range word, and the
    BN-backward sums against the sums of its own output (one slab row per ring workgroup)."""
    convt_ring(2)
    x2_convT_ring_case(cin, cout, n, h, w)


@pytest.mark.parametrize("slack", SLACKS)
def test_x2_convT_ring_loose_words(slack, convt_ring):
    convt_ring(2)
    x2_convT_ring_case(512, 256, 1, 16, 32, slack=slack)


def x2_convT_ring_case(cin, cout, n, h, w, signed=False, slack=1.0):
    r = _convT_x2_pair(cin, cout, n, h, w, seed=60, signed=signed, slack=slack)
    a = torch.relu(r["x"] * r["s"].view(1, -1, 1, 1) + r["t"].view(1, -1, 1, 1)).double().requires_grad_()
    if signed:
        check_signed_inputs(r["s"], a.detach())
        check_signed_inputs(r["sc"], torch.relu(r["yprev"] * r["sc"] + r["sh"]))
    y = F.conv_transpose2d(a, r["wt"].double(), r["b"].double(), stride=2)
    (ga,) = torch.autograd.grad(y, (a,), r["dy"].double())
    assert rel(nchw(r["up"].cpu(), n, 2 * h, 2 * w), y.detach()) < TOL
    assert r["amu"].item() == r["up"].abs().max().item()
    assert rel(nchw(r["da"].cpu(), n, h, w), ga) < TOL
    assert r["amo"].item() == r["da"].abs().max().item()
    M = n * h * w
    blocks = cin // 256
    assert r["rows"] == min(M // 256, max(1, 256 // blocks))  # the ring kernel's workgroup rows
    y64, sc, sh = r["yprev"].double(), r["sc"].double(), r["sh"].double()
    g64 = r["da"].double() * (y64 * sc + sh > 0).double()
    xh = (y64 - r["mean"].double()) * r["invstd"].double()
    got = r["slab"].double().sum(0)
    for k, term in enumerate([g64, g64 * xh, xh]):
        err = (got[k] - term.sum(0)).abs() / (term.abs().sum(0) + 1e-30)
        assert float(err.max()) < 1e-6, (k, float(err.max()))


@pytest.mark.parametrize("mode", [1, 2])
def test_x2_convT_ring_plain_operands(mode, convt_ring):
    """The ring kernel without the optional parts: a forward source with no BN+ReLU transform and no bias,
    a data gradient with no BN-backward sums (no slab) — against torch in fp64, with both range words."""
    convt_ring(mode)
    cin, cout, n, h, w = 256, 128, 2, 32, 32
    x = gen(n, cin, h, w, seed=81)
    wt = gen(cin, cout, 2, 2, seed=82, scale=0.05)
    dy = gen(n, cout, 2 * h, 2 * w, seed=83)
    fwd, dg = pack_convT_x2(wt)
    d = lambda t_: t_.to(DEV).contiguous()  # noqa: E731
    xd, dud = d(nhwc(x)), d(nhwc(dy))
    M = n * h * w
    up = torch.empty(4 * M, cout, device=DEV)
    amu, amo = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ep = K.Epilogue(K.ptr(up), None, None, None, K.EP_SCATTER2X, 0)
    ep.amax = K.ptr(amu)
    K.call("selunet_gemm_gather_x2", K.gather(n, h, w, 1, K.source(xd, cin)), K.ptr(fwd), 4 * cout, cin, ep,
           K.ptr(word(x.abs().max())), None, K.stream_ptr())
    da = torch.empty(M, cin, device=DEV)
    ep = K.Epilogue(K.ptr(da), None, None, None, K.EP_PLAIN, 0)
    ep.amax = K.ptr(amo)
    K.call("selunet_gemm_gather_x2", K.gather(n, h, w, 4, K.source(dud, cout)), K.ptr(dg), cin, 4 * cout, ep,
           K.ptr(word(dy.abs().max())), None, K.stream_ptr())
    torch.cuda.synchronize()
    a = x.double().requires_grad_()
    y = F.conv_transpose2d(a, wt.double(), None, stride=2)
    (ga,) = torch.autograd.grad(y, (a,), dy.double())
    assert rel(nchw(up.cpu(), n, 2 * h, 2 * w), y.detach()) < TOL
    assert rel(nchw(da.cpu(), n, h, w), ga) < TOL
    assert amu.item() == up.abs().max().item() and amo.item() == da.abs().max().item()


@pytest.mark.parametrize("cin,cout,n,h,w", [
    (512, 256, 4, 32, 32),
    (256, 128, 4, 128, 160),  # data gradient: 320 row tiles on 256 workgroups (two tiles for some)
    (512, 256, 16, 32, 96),   # forward: 4 column blocks x 64 workgroup rows over 192 row tiles
])
@pytest.mark.parametrize("mode", [1, 2])  # 2 (default): the forward on 8 x 1 waves
def test_x2_convT_ring_matches_resident(cin, cout, n, h, w, mode, convt_ring):
    """The ring kernel computes the products and sums of the resident-weight / staged kernels in the same
    order (hl, lh, hh per 16-k step, k ascending): forward and data gradient outputs bit-identical with
    SELUNET_OPT_CONVT_RING on and off, also where workgroups walk several row tiles."""
    convt_ring(0)
    off = _convT_x2_pair(cin, cout, n, h, w, seed=70)
    convt_ring(mode)
    on = _convT_x2_pair(cin, cout, n, h, w, seed=70)
    assert torch.equal(on["up"], off["up"])
    assert torch.equal(on["da"], off["da"])
    assert on["amu"].item() == off["amu"].item() and on["amo"].item() == off["amo"].item()
    sums = lambda r: r["slab"].double().sum(0)  # noqa: E731
    assert rel(sums(on), sums(off)) < 1e-6


@pytest.mark.parametrize("cin,cout", [(512, 256), (128, 64), (256, 128)])
@pytest.mark.parametrize("n,h,w", [(2, 13, 18), (2, 9, 32), (1, 6, 64)])  # w % 32 == 0: one dU decode per stage
def test_x2_convT_wgrad(cin, cout, n, h, w):
    """ConvTranspose2d weight gradient through selunet_gemm_wgrad_x2 (split partials reduced into the
    [ci][co][2][2] layout) against torch in fp64; bit-reproducible."""
    x2_convT_wgrad_case(cin, cout, n, h, w)


@pytest.mark.parametrize("slack", SLACKS)
def test_x2_convT_wgrad_loose_words(slack):
    x2_convT_wgrad_case(128, 64, 2, 13, 18, slack=slack)


def x2_convT_wgrad_case(cin, cout, n, h, w, signed=False, slack=1.0):
    x = gen(n, cin, h, w, seed=13)
    s, t = bn_fold(cin, 30, signed)
    a = torch.relu(x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)).double()
    if signed:
        check_signed_inputs(s, a)
    wt = gen(cin, cout, 2, 2, seed=14, scale=0.05).double().requires_grad_()
    y = F.conv_transpose2d(a, wt, None, stride=2)
    dy = gen(*y.shape, seed=16) * 1e-8
    (gw,) = torch.autograd.grad(y, (wt,), dy.double())
    d = lambda t_: t_.to(DEV).contiguous()  # noqa: E731
    xd, sd, td, dud = d(nhwc(x)), d(s), d(t), d(nhwc(dy))
    amp, amq = word(a.abs().max() * slack), word(dy.abs().max() * slack)
    gp = K.gather(n, h, w, 1, K.source(xd, cin, sd, td))
    gq = K.gather(n, h, w, 4, K.source(dud, cout))
    wsb = K.query("selunet_gemm_wgrad_x2_ws_bytes", gp, gq)
    assert wsb > 0
    ws = torch.empty(wsb // 4, device=DEV)
    outs = []
    for _ in range(2):
        out = torch.full((cin, cout, 2, 2), float("nan"), device=DEV)
        K.call("selunet_gemm_wgrad_x2", gp, gq, K.ptr(ws), wsb, K.WG_CONVT, K.ptr(out), K.ptr(amp), None, K.ptr(amq),
               None, K.stream_ptr())
        outs.append(out)
    torch.cuda.synchronize()
    assert rel(outs[0].cpu(), gw) < TOL
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("n,h,w", [(2, 128, 160), (3, 100, 96), (1, 70, 64)])
def test_x2_convT_wgrad_deep(n, h, w):
    """unpool1's shape class (128 x 256 tiles, gemm_wgrad_x2_kernel<128, 256, 512>) over splits of many 32-pixel
    stages, ragged last stages and odd / even stage counts per split."""
    x2_convT_wgrad_case(128, 64, n, h, w)
