"""Every consumer of the folded BatchNorm transform relu(v*scale[c] + shift[c]) at signed scales.

Trained networks have BatchNorm gammas of both signs and near zero; every other test here folds with
scale = |N(0, 1)| + 0.5. These cases run the existing tests' bodies (same shapes — the smallest each test uses —
same fp64 CPU references, same tolerances) with tests/test_gpu_kernels.bn_fold(signed=True) / bn_state: scale ~
N(0, 1) with channels [0, 4) negative, [4, 8) and one more exactly zero, shift ~ 0.5 N(0, 1), and in the backward
tests coef[0] = k0 = gamma*invstd of the same gamma as the ReLU mask's scale. Each case asserts on its own inputs
that at least 25 % of the channels have a negative scale and that the reference's ReLU is active on 10 % to 90 % of
its elements (check_signed_inputs) before it looks at the kernel.

What a wrong kernel would do here and not elsewhere: a ReLU mask on raw y, or on y*|scale|; a max-pool argmax on
raw y (a negative scale reverses the order); a scale hoisted out of a max; a range bound without its |gamma|.

New references (the operations had none at kernel level): the max-pool under a general transform, the heads'
forward, the BN-backward applies against the fp64 formula. Their bounds are derived in the docstrings.
"""
import pytest
import torch

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from tests import test_gpu_apply_fused as AF
from tests import test_gpu_convt_bf16 as CB
from tests import test_gpu_kernels as KT
from tests import test_gpu_wino as WI
from tests import test_gpu_x2 as X2
from tests.test_gpu_apply_fused import check_dy_fp64
from tests.test_gpu_kernels import (bn_fold, bn_state, check_bnb_sums, check_signed_inputs, gather_wgs,  # noqa: F401
                                    gen, halo_wgs, kernel_option, nchw, nhwc, rel, signed_gamma)
from tests.test_gpu_x2 import convt_ring, tile_queue, x2d  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DTYPES = [torch.float32, BF]
X2_VARIANTS = [(1, 0), (0, 0), (0, 1), (0, 2)]


def test_signed_fold_helper():
    """bn_fold(signed=True) / bn_state: the overrides are there, the default is what it always was."""
    for c, seed in ((32, 10), (64, 12), (512, 30)):
        s, t = bn_fold(c, seed, signed=True)
        assert bool((s[:4] < 0).all()) and bool((s[4:8] == 0).all()) and int((s == 0).sum()) == 5
        assert float((s < 0).float().mean()) >= 0.25 and bool((s > 0).any())
        s0, t0 = bn_fold(c, seed)
        assert torch.equal(s0, gen(c, seed=seed).abs() + 0.5) and torch.equal(t0, gen(c, seed=seed + 1) * 0.3)
        st = bn_state(c, seed, True)
        assert torch.equal(st["scale"], st["gamma"] * st["invstd"]) and torch.equal(st["k0"], st["scale"])
        assert bool((st["invstd"] > 0).all()) and torch.equal(torch.sign(st["scale"]), torch.sign(st["gamma"]))


# ------------------------------------------------------------------ 3x3 forward with statistics
@pytest.mark.parametrize("cin0,cin1,cout,n,h,w", [
    (64, 0, 64, 2, 16, 16),      # persistent halo kernel
    (64, 64, 128, 2, 8, 8),      # two sources, gather fallback (below the halo tile)
    (64, 64, 128, 1, 16, 48),    # two sources, halo kernel
    (32, 0, 64, 2, 24, 20),      # single-chunk halo kernel
])
@pytest.mark.parametrize("wgs", [0, 3])
def test_conv3x3_fwd_stats_signed(cin0, cin1, cout, n, h, w, wgs, halo_wgs):
    halo_wgs(wgs)
    KT.conv3x3_fwd_stats_case(cin0, cin1, cout, n, h, w, True, signed=True)


@pytest.mark.parametrize("cin0,cin1,cout,n,h,w", [(64, 0, 64, 2, 40, 36), (128, 128, 256, 1, 33, 40)])
@pytest.mark.parametrize("wgs", [0, 3])
def test_conv3x3_bf16_persist_fwd_stats_signed(cin0, cin1, cout, n, h, w, wgs, halo_wgs):
    halo_wgs(wgs)
    KT.conv3x3_bf16_persist_fwd_stats_case(cin0, cin1, cout, n, h, w, signed=True)


@pytest.mark.parametrize("wgs", [0, 3])
def test_wino_fwd_stats_signed(wgs, halo_wgs):
    halo_wgs(wgs)
    WI.wino_fwd_stats_case(64, 0, 64, 2, 16, 16, True, signed=True)


@pytest.mark.parametrize("cin0,cin1,cout,n,h,w", [(64, 0, 64, 2, 16, 16), (64, 64, 128, 1, 16, 48)])
@pytest.mark.parametrize("wgs", [0, 3])
@pytest.mark.parametrize("x2d_mode,tq", X2_VARIANTS)
def test_x2_fwd_stats_signed(cin0, cin1, cout, n, h, w, wgs, x2d_mode, tq, halo_wgs, x2d, tile_queue):
    halo_wgs(wgs)
    x2d(x2d_mode)
    tile_queue(tq)
    X2.x2_fwd_stats_case(cin0, cin1, cout, n, h, w, True, signed=True)


# ------------------------------------------------------------------ ConvTranspose forward from a BN source
@pytest.mark.parametrize("gwgs", [-1, 3])
def test_convT_fwd_bwd_signed(gwgs, gather_wgs):
    """SCATTER2X forward, and the weight gradient with the transformed operand (atomic, split-partials and the
    ConvTranspose2d-layout reduction)."""
    gather_wgs(gwgs)
    KT.convT_fwd_bwd_case(128, 64, signed=True)


def test_convT_bf16_fwd_signed(convt_ring):
    convt_ring(0)
    CB.convT_bf16_fwd_case(128, 64, 2, 9, 64, signed=True)


@pytest.mark.parametrize("gwgs", [-1, 3])
def test_x2_convT_fwd_dgrad_signed(gwgs, gather_wgs):
    """Forward from a signed BN source; the data gradient's BN-backward sums at a signed fold."""
    gather_wgs(gwgs)
    X2.x2_convT_fwd_dgrad_case(128, 64, signed=True)


def test_x2_convT_ring_signed(convt_ring):
    convt_ring(2)
    X2.x2_convT_ring_case(512, 256, 1, 16, 32, signed=True)


# ------------------------------------------------------------------ weight gradients with transformed operands
@pytest.mark.parametrize("cin0,cin1,cout", [(64, 0, 64), (64, 64, 128)])
def test_conv3x3_wgrad_signed(cin0, cin1, cout):
    """selunet_gemm_wgrad, selunet_gemm_wgrad_ws and selunet_gemm_wgrad_ws_to (Conv2d layout), fp32."""
    KT.conv3x3_wgrad_case(cin0, cin1, cout, True, False, 16, 16, signed=True)


def test_conv3x3_bf16_fwd_wgrad_signed():
    KT.conv3x3_bf16_fwd_wgrad_case(64, 0, 64, False, 16, 16, signed=True)


def test_convT_bf16_wgrad_signed():
    """bf16 ConvTranspose2d weight gradient whose x operand is a signed BN+ReLU source (the existing bf16 test
    has no transform): selunet_gemm_wgrad, selunet_gemm_wgrad_ws and selunet_gemm_wgrad_ws_to (ConvTranspose2d
    layout) against torch in fp64 on the bf16-rounded operands, test_convT_bf16_wgrad's bound and smallest shape."""
    n, h, w, cin, cout = 2, 6, 10, 64, 64
    x = KT._bf(gen(n, cin, h, w, seed=45))
    s, t = bn_fold(cin, 160, signed=True)
    a = KT._bf(torch.relu(x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)))  # the stager's bf16 operand
    check_signed_inputs(s, a)
    wt = gen(cin, cout, 2, 2, seed=46, scale=0.05).double().requires_grad_()
    y = torch.nn.functional.conv_transpose2d(a.double(), wt, stride=2)
    dy = KT._bf(gen(*y.shape, seed=47))
    (gw,) = torch.autograd.grad(y, wt, dy.double())
    xd, dud, sd, td = nhwc(x).to(DEV).bfloat16(), nhwc(dy).to(DEV).bfloat16(), s.to(DEV), t.to(DEV)
    gp, gq = K.gather(n, h, w, 1, K.source(xd, cin, sd, td)), K.gather(n, h, w, 4, K.source(dud, cout))
    ld = K.query("selunet_wgrad_ld", 4 * cout)
    packed = torch.zeros(cin, ld, device=DEV)
    K.call("selunet_gemm_wgrad", gp, gq, K.ptr(packed), K.BF16, K.stream_ptr())
    det = KT.wgrad_ws(gp, gq, packed)
    for buf in (packed, det):
        gwd = torch.empty(cin, cout, 2, 2, device=DEV)
        K.call("selunet_unpack_convT_grad", K.ptr(buf), cin, cout, K.ptr(gwd), K.stream_ptr())
        assert rel(gwd.cpu(), gw) < 1e-3
    wsb = K.query("selunet_gemm_wgrad_ws_bytes", gp, gq, K.BF16)
    assert wsb > 0
    ws = torch.empty(wsb // 4, device=DEV)
    to = torch.full((cin, cout, 2, 2), float("nan"), device=DEV)
    K.call("selunet_gemm_wgrad_ws_to", gp, gq, None, K.ptr(ws), wsb, K.WG_CONVT, K.ptr(to), K.BF16, K.stream_ptr())
    assert rel(to.cpu(), gw) < 1e-3


def test_wino_wgrad_signed():
    WI.wino_wgrad_case(64, 0, 64, True, 2, 16, 16, signed=True)


@pytest.mark.parametrize("wgs", [-1, 4])
@pytest.mark.parametrize("nw", [12, 8])
@pytest.mark.parametrize("tw", [16, 8])
def test_wino_wgrad_signed_variants(tw, nw, wgs, kernel_option):
    """The four instantiations of the Winograd weight gradient (tile width, waves) with signed scales, one tile
    per workgroup and several (WGRAD_WGS = 4 at 2x20x36: 18 tiles as 5, 5, 5, 3 at tile width 16; 30 as
    8, 8, 8, 6 at 8)."""
    for name, v in (("WINO_WGRAD_TW", tw), ("WINO_WGRAD_WAVES", nw), ("WGRAD_WGS", wgs)):
        kernel_option((name, v))
        assert K.set_option(name, v) == v
    WI.wino_wgrad_case(64, 0, 64, True, 2, 20, 36, signed=True)


@pytest.mark.parametrize("cin0,cin1,cout", [(64, 0, 64), (64, 64, 128)])
def test_x2_wgrad_signed(cin0, cin1, cout):
    X2.x2_wgrad_case(cin0, cin1, cout, True, 2, 16, 16, signed=True)


def test_x2_convT_wgrad_signed():
    X2.x2_convT_wgrad_case(128, 64, 2, 13, 18, signed=True)


# ------------------------------------------------------------------ BN-backward sums
def test_bn_forward_backward_signed():
    """selunet_bn_finalize, selunet_bn_bwd_reduce, selunet_bn_bwd_finalize and selunet_bn_bwd_apply against
    torch's autograd through batch_norm + relu with a signed gamma."""
    KT.bn_forward_backward_case(signed=True)


@pytest.mark.parametrize("h", [8, 32])  # gather GEMM, halo kernel
@pytest.mark.parametrize("wgs", [0, 3])
def test_conv3x3_dgrad_bnb_signed(h, wgs, halo_wgs, gather_wgs):
    halo_wgs(wgs)
    gather_wgs(wgs - 2 if wgs else -1)
    KT.conv3x3_dgrad_case(64, 64, 0, h, h, signed=True)


def test_conv3x3_bf16_dgrad_bnb_signed():
    KT.conv3x3_bf16_persist_dgrad_case(64, 64, 0, 20, 40, signed=True)


def test_wino_dgrad_bnb_signed():
    WI.wino_dgrad_case(64, 64, 0, 32, 32, signed=True)


@pytest.mark.parametrize("x2d_mode,tq", X2_VARIANTS)
def test_x2_dgrad_bnb_signed(x2d_mode, tq, x2d, tile_queue):
    x2d(x2d_mode)
    tile_queue(tq)
    X2.x2_dgrad_case(64, 64, 0, 32, 32, signed=True)


# ------------------------------------------------------------------ fused BN-backward applies
def test_wgrad_x2_bn_signed():
    """selunet_conv3x3_wgrad_x2_bn: both operands from signed folds; dy also against the fp64 formula."""
    AF.wgrad_x2_bn_case(64, 64, signed=True)


def heads_da(r, dt):
    """dA [m][64] = sum_h g_h[m] w_h[c] in fp64, rounded to the activation dtype as the producer stores it."""
    da = sum(g.double().cpu()[:, None] * r["w"][i].double().cpu()[None, :] for i, g in enumerate(r["g"]))
    return da.float().to(dt).double()


def pool_ref(y, sc, sh, n, h, w):
    """fp64 relu(y*scale + shift) as windows [n][h/2][w/2][c][4] (row-major inside the window) and the index of
    each window's first maximum (strict >, row-major: ATen's max_pool2d on the transformed values)."""
    c = y.shape[1]
    z = torch.relu(y.double().cpu() * sc.double().cpu() + sh.double().cpu()).reshape(n, h // 2, 2, w // 2, 2, c)
    win = z.permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    best, idx = win[..., 0], torch.zeros(win.shape[:-1], dtype=torch.long)
    for k in (1, 2, 3):
        up = win[..., k] > best
        best, idx = torch.where(up, win[..., k], best), torch.where(up, k, idx)
    return win, idx


def pool_route(dp, idx, n, h, w):
    """dpool [n*h/2*w/2][c] routed to position idx of each window: [n*h*w][c] in fp64."""
    c = dp.shape[1]
    g = torch.zeros(n, h // 2, w // 2, c, 4, dtype=torch.float64)
    g.scatter_(4, idx[..., None], dp.double().cpu().reshape(n, h // 2, w // 2, c, 1))
    return g.reshape(n, h // 2, w // 2, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n * h * w, c)


@pytest.mark.parametrize("form", ["pool", "pool_noskip", "heads1", "heads3"])
def test_wgrad_x2_bn_src_signed(form):
    """selunet_conv3x3_wgrad_x2_bn_src and selunet_bn_bwd_apply_pool / _heads: as the unsigned test, and the
    standalone apply's dy against the fp64 formula on the fp64 dA (y is coarse: its pool windows tie exactly or
    differ by at least 0.5 |scale|, so the routing is the same in any arithmetic)."""
    r = AF.wgrad_x2_bn_src_case(form, signed=True)
    n, h, w, c = r["shape"]
    if form.startswith("pool"):
        dp, ds = r["keep"]
        _, idx = pool_ref(r["y"], r["bn"][0], r["bn"][1], n, h, w)
        da = pool_route(dp, idx, n, h, w) + (ds.double().cpu() if ds is not None else 0.0)
    else:
        wt, g = r["keep"]
        nh = int(form[-1])
        da = heads_da(dict(w=wt, g=g[:nh]), torch.float32)
    check_dy_fp64(r["dy"], r["amax"], da, r["y"], r["bn"], torch.float32)


@pytest.mark.parametrize("dt,cin,n,h,w", [(torch.float32, 3, 2, 32, 32), (BF, 3, 2, 32, 48)])
def test_first_conv_wgrad_bn_signed(dt, cin, n, h, w):
    KT.first_conv_wgrad_bn_case(dt, cin, n, h, w, signed=True)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("form", [1, 2, 3])
def test_apply_forms_signed(dt, form):
    """selunet_bn_bwd_apply_amax in every SELUNET_OPT_APPLY_U8 form (0 and `form`, bit-identical) against fp64."""
    r = AF.apply_forms_case(dt, 64, form, signed=True)
    check_dy_fp64(r["dy"], r["amax"], r["da"], r["y"], r["bn"], dt)


def check_head_sums(slab, g, y, sc, sh, dt):
    """The heads' weight / bias gradient sums [rows][nh][65] against fp64 sum g*z, sum g with z = relu(y*scale +
    shift) formed from y as stored, to the 1e-4 of the tensor's maximum this suite's fp32 kernels are held to
    (tests/test_gpu_kernels.TOL)."""
    z = torch.relu(y.double().cpu() * sc.double().cpu() + sh.double().cpu())
    want = torch.cat([torch.cat([(gi.double().cpu()[:, None] * z).sum(0), gi.double().cpu().sum().reshape(1)])
                      for gi in g])
    got = slab.double().sum(0).reshape(-1)[:want.numel()]
    assert rel(got, want) < KT.TOL


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nh", [1, 3])
def test_apply_heads_signed(dt, nh):
    """selunet_heads_bwd (storing and sums-only, with the BN-backward sums) and selunet_bn_bwd_apply_heads."""
    r = AF.apply_heads_case(dt, nh, signed=True)
    da = heads_da(r, dt)
    sc, sh, mean, invstd, _ = r["bn"]
    check_bnb_sums(r["bslab"], da, r["y"].double().cpu(), sc.cpu(), sh.cpu(), mean.cpu(), invstd.cpu(),
                   tol=1e-5 if dt == torch.float32 else 1e-4)
    check_head_sums(r["slab"], r["g"], r["y"], sc, sh, dt)
    check_dy_fp64(r["dy"], r["amax"], da, r["y"], r["bn"], dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_apply_heads_planes_signed(dt):
    """selunet_heads_bwd_planes (storing and sums-only) and selunet_bn_bwd_apply_heads_planes."""
    r = AF.apply_heads_planes_case(dt, signed=True)
    da = heads_da(r, dt)
    sc, sh, mean, invstd, _ = r["bn"]
    check_bnb_sums(r["bslab"], da, r["y"].double().cpu(), sc.cpu(), sh.cpu(), mean.cpu(), invstd.cpu(),
                   tol=1e-5 if dt == torch.float32 else 1e-4)
    check_head_sums(r["slab"], r["g"], r["y"], sc, sh, dt)
    check_dy_fp64(r["dy"], r["amax"], da, r["y"], r["bn"], dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("skip", [True, False])
def test_apply_pool_signed(dt, skip):
    """selunet_maxpool2_bwd (storing and sums-only, with the BN-backward sums) and selunet_bn_bwd_apply_pool:
    dA = route(dpool) + dskip rounded to the activation dtype, from the fp64 routing (coarse y: exact ties or
    gaps of at least 0.5 |scale|)."""
    r = AF.apply_pool_case(dt, 64, skip, signed=True)
    n, h, w, c = r["shape"]
    sc, sh, mean, invstd, _ = r["bn"]
    _, idx = pool_ref(r["y"], sc, sh, n, h, w)
    da = pool_route(r["dp"], idx, n, h, w) + (r["ds"].double().cpu() if skip else 0.0)
    da = da.float().to(dt).double()
    check_bnb_sums(r["bslab"], da, r["y"].double().cpu(), sc.cpu(), sh.cpu(), mean.cpu(), invstd.cpu(),
                   tol=1e-5 if dt == torch.float32 else 1e-4)
    check_dy_fp64(r["dy"], r["amax"], da, r["y"], r["bn"], dt)


# ------------------------------------------------------------------ max-pool under a general transform
@pytest.mark.parametrize("dt", DTYPES)
def test_maxpool_signed_transform(dt):
    """selunet_maxpool2_fwd / _bwd with a signed fold (the existing test runs scale = 1, shift = 0 and asserts
    bit equality; v*scale + shift may contract to an FMA here).

    Forward against fp64 max over relu(y*scale + shift): 1e-6 of the maximum (one fp32 multiply-add, 2^-23 of
    |y*scale| + |shift| <= 2 max at most), plus the bf16 unit roundoff (8 significant bits: 2^-8) where the output
    is stored in bf16 (y is rounded to bf16 before the reference).
    Routing: dz = route(dpool to the first maximum, row-major) + dskip against the fp64 routing, same bound.
    Exact ties stay exact under any transform: duplicated raw y, zero-scale channels (every value is the shift)
    and all-dead windows (every value 0 after the ReLU) go to the first position. Windows left out of the dz
    comparison: the two largest fp64 transformed values differ by less than 1e-5 relative without being such an
    exact tie, or a value lies within 1e-6 of the ReLU threshold; at most 0.1 % of the windows.
    Channels [0, 4) have a negative scale and a shift that keeps them active, so the transformed argmax is the raw
    minimum: it differs from the raw-y argmax in most of their windows (asserted on the reference), which is
    what a kernel that pooled raw y would get wrong."""
    n, c, h, w = 2, 64, 8, 12
    code = K.dtype_code(dt)
    y = gen(n, c, h, w, seed=117)
    y[:, :, ::2, 1::2] = y[:, :, ::2, ::2]          # exact tie between (0,0) and (0,1) in every window
    y = y.to(dt).float()
    s, t = bn_fold(c, 118, signed=True)
    t[:4] = 3.0 * s[:4].abs()                        # negative scale, active for y < 3: order reversed
    yd = nhwc(y).to(dt).to(DEV)
    sd, td = s.to(DEV), t.to(DEV)
    win, idx = pool_ref(yd.float(), sd, td, n, h, w)
    check_signed_inputs(s, win)
    # the reference's own conditions
    yw = nhwc(y).double().reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    raw_idx = pool_ref(yd.float(), torch.ones(c), torch.full((c,), 10.0), n, h, w)[1]  # argmax of raw y (+10 > 0)
    assert float((raw_idx[..., :4] != idx[..., :4]).double().mean()) > 0.5
    assert bool((win.amax(-1) == 0).any())            # all-dead windows exist
    top2 = win.topk(2, dim=-1).values
    i2 = win.topk(2, dim=-1).indices
    close = (top2[..., 0] - top2[..., 1]) < 1e-5 * top2[..., 0]
    y_tie = torch.gather(yw, -1, i2[..., :1]) == torch.gather(yw, -1, i2[..., 1:])
    exact = y_tie[..., 0] | (s == 0).view(1, 1, 1, c)
    v = yw * s.double().view(1, 1, 1, c, 1) + t.double().view(1, 1, 1, c, 1)
    near = (v.abs() <= 1e-6 * ((yw * s.double().view(1, 1, 1, c, 1)).abs() + t.double().abs().view(1, 1, 1, c, 1)))
    near = near.any(-1) & ~(s == 0).view(1, 1, 1, c)
    excluded = (close & ~exact) | near
    assert float(excluded.double().mean()) <= 1e-3, float(excluded.double().mean())
    tol = 1e-6 + (2.0 ** -8 if dt == BF else 0.0)
    # forward
    out = torch.empty(n * h * w // 4, c, dtype=dt, device=DEV)
    K.call("selunet_maxpool2_fwd", K.ptr(yd), n, h, w, c, K.ptr(sd), K.ptr(td), K.ptr(out), code, K.stream_ptr())
    torch.cuda.synchronize()
    ref = win.amax(-1).reshape(-1, c)
    assert rel(out.float().cpu(), ref) < tol
    # backward: storing, storing with the BN-backward sums, sums only
    dp = gen(n * h * w // 4, c, seed=119).to(dt).to(DEV)
    ds = gen(n * h * w, c, seed=120).to(dt).to(DEV)
    mean, invstd = (gen(c, seed=121) * 0.1).to(DEV), (gen(c, seed=122).abs() + 0.5).to(DEV)
    keep = (~excluded).reshape(n, h // 2, 1, w // 2, 1, c).expand(n, h // 2, 2, w // 2, 2, c).reshape(n * h * w, c)
    for skip in (True, False):
        want = pool_route(dp, idx, n, h, w) + (ds.double().cpu() if skip else 0.0)
        dz = torch.full((n * h * w, c), float("nan"), dtype=dt, device=DEV)
        K.call("selunet_maxpool2_bwd", K.ptr(yd), n, h, w, c, K.ptr(sd), K.ptr(td), K.ptr(dp),
               K.ptr(ds) if skip else None, K.ptr(dz), None, code, K.stream_ptr())
        torch.cuda.synchronize()
        got = dz.double().cpu()
        assert not torch.isnan(got).any()
        assert float(((got - want).abs() * keep).max() / want.abs().max()) < tol
        rows = K.query("selunet_maxpool2_bwd_slab_rows", n, h, w, c)
        slabs = []
        for store in (True, False):
            slab = torch.full((rows, 3, c), float("nan"), device=DEV)
            bnb = K.BnBwdStats(K.ptr(yd), K.ptr(sd), K.ptr(td), K.ptr(mean), K.ptr(invstd), K.ptr(slab))
            dz2 = torch.full_like(dz, float("nan")) if store else None
            K.call("selunet_maxpool2_bwd", K.ptr(yd), n, h, w, c, K.ptr(sd), K.ptr(td), K.ptr(dp),
                   K.ptr(ds) if skip else None, K.ptr(dz2), bnb, code, K.stream_ptr())
            torch.cuda.synchronize()
            if store:
                assert torch.equal(dz2, dz)
            slabs.append(slab.cpu())
        assert torch.equal(slabs[0], slabs[1])
        # (the sums of the kernel's own dz: every window, the near-ties included)
        check_bnb_sums(slabs[0], got, yd.double().cpu(), s, t, mean.cpu(), invstd.cpu(),
                       tol=1e-5 if dt == torch.float32 else 1e-4)


# ------------------------------------------------------------------ heads forward
def heads_inputs(dt, seed, nk):
    m = 3 * 4096 + 77  # ragged tail
    y = gen(m, 64, seed=seed).to(dt)
    s, t = bn_fold(64, seed + 1, signed=True)
    wt, b = gen(nk, 64, seed=seed + 3) * 0.2, gen(nk, seed=seed + 4)
    z = torch.relu(y.double() * s.double() + t.double())
    check_signed_inputs(s, z)
    return m, y, s, t, wt, b, z @ wt.double().T + b.double()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nh", [1, 3])
def test_heads_fwd_signed(dt, nh):
    """selunet_heads_fwd (conv1x1 / conv_select / conv_aux on relu(bn(y)), C = 64) against relu(y*s + t) @ w.T + b
    in fp64: 1e-6 of the output's maximum (a 64-term fp32 dot product and the transform's multiply-add: well under
    66 * 2^-24 = 4e-6 of sum |terms| in the worst case, 1e-6 of the maximum at random signs); bf16: y rounded to
    bf16 first, same bound (the outputs are fp32)."""
    m, y, s, t, wt, b, ref = heads_inputs(dt, 130, nh)
    yd, sd, td, wd, bd = (x.to(DEV).contiguous() for x in (y, s, t, wt, b))
    outs = [torch.full((m,), float("nan"), device=DEV) for _ in range(nh)]
    K.call("selunet_heads_fwd", K.ptr(yd), m, K.ptr(sd), K.ptr(td), K.ptr(wd), K.ptr(bd), nh,
           *[K.ptr(outs[i]) if i < nh else None for i in range(3)], K.dtype_code(dt), K.stream_ptr())
    torch.cuda.synchronize()
    got = torch.stack(outs, 1).double().cpu()
    assert not torch.isnan(got).any()
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-6


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nk", [3, 8])
def test_heads_fwd_planes_signed(dt, nk):
    """selunet_heads_fwd_planes: nk outputs written as the channel planes of an NCHW [5, nk, hw] tensor; the
    reference and bound of test_heads_fwd_signed."""
    m, y, s, t, wt, b, ref = heads_inputs(dt, 140, nk)
    n_img, hw = 5, m // 5
    assert n_img * hw == m
    yd, sd, td, wd, bd = (x.to(DEV).contiguous() for x in (y, s, t, wt, b))
    out = torch.full((n_img, nk, hw), float("nan"), device=DEV)
    hp = K.HeadPlanes()
    hp.n, hp.hw = nk, hw
    for k in range(nk):
        hp.plane[k] = out.data_ptr() + k * hw * 4
        hp.img_stride[k] = nk * hw
    K.call("selunet_heads_fwd_planes", K.ptr(yd), m, K.ptr(sd), K.ptr(td), K.ptr(wd), K.ptr(bd), hp,
           K.dtype_code(dt), K.stream_ptr())
    torch.cuda.synchronize()
    got = out.permute(0, 2, 1).reshape(m, nk).double().cpu()
    assert not torch.isnan(got).any()
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-6


# ------------------------------------------------------------------ range bounds
@pytest.mark.parametrize("c", [64, 256])
def test_finalize_centered_bound_signed(c):
    """selunet_bn_stats_finalize_centered_bound with signed gamma / beta (exact zero gammas among them): the
    folded scale carries gamma's sign (zero stays zero), and the range word equals max_c (|gamma_c| sqrt(count) +
    |beta_c|) * 1.0001 (to 2e-4, as tests/test_gpu_bn_shift.py holds it) and covers the true max |relu(bn(y))|,
    also on a batch with one outlier per channel, which comes close to Samuelson's sqrt(count - 1)."""
    M = 4096
    g = torch.Generator().manual_seed(151)
    y = torch.randn(M, c, generator=g, dtype=torch.float64) * 0.7 + 0.4
    y[0] = 60.0  # one outlier per channel (xhat = 0.8 sqrt(M)), below the mean in the odd channels
    y[0, 1::2] = -60.0
    gamma, beta = signed_gamma(c, 152), gen(c, seed=153) * 0.5
    gamma[1], beta[9] = -1.5 * gamma.abs().max(), -1.5 * beta.abs().max()  # the largest magnitudes are negative
    m64, v64 = y.mean(0), y.var(0, unbiased=False)
    center = (m64 + 0.1).float()
    d = y - center.double()
    slab = torch.stack([d.sum(0), (d * d).sum(0)]).reshape(1, 2, c).float().to(DEV).contiguous()
    ws = torch.empty(K.query("selunet_reduce_ws_bytes", 2 * c) // 8, dtype=torch.float64, device=DEV)
    cd, gd, bd = center.to(DEV), gamma.to(DEV), beta.to(DEV)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    mean, invstd, scale, shift = (torch.full((c,), float("nan"), device=DEV) for _ in range(4))
    bound = torch.zeros(1, device=DEV)
    K.call("selunet_bn_stats_finalize_centered_bound", K.ptr(slab), 1, K.ptr(ws), None, M, c, K.ptr(cd), None,
           K.ptr(gd), K.ptr(bd), K.ptr(rm), K.ptr(rv), K.ptr(nbt), 0.1, 1e-5, K.ptr(mean), K.ptr(invstd),
           K.ptr(scale), K.ptr(shift), K.ptr(bound), K.stream_ptr())
    torch.cuda.synchronize()
    sc, sh = scale.double().cpu(), shift.double().cpu()
    act = torch.relu(y * sc + sh)
    check_signed_inputs(sc, act)
    assert torch.equal(torch.sign(scale.cpu()), torch.sign(gamma)) and bool((invstd > 0).all())
    want_sc = gamma.double() / (v64 + 1e-5).sqrt()
    assert float((sc - want_sc).abs().max() / want_sc.abs().max()) < 1e-5
    want = float((gamma.double().abs() * M ** 0.5 + beta.double().abs()).max()) * 1.0001
    assert abs(bound.item() - want) <= 2e-4 * want
    true_max = float(torch.relu((y - m64) / (v64 + 1e-5).sqrt() * gamma.double() + beta.double()).max())
    assert 0 < true_max <= bound.item() and float(act.max()) <= bound.item()
    assert true_max > 0.5 * float(gamma.abs().max()) * M ** 0.5  # the batch does come close to the bound
