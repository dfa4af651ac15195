"""The pointwise kernels of csrc/pointwise.hip at sizes where their loops iterate, wrap and cap.

Every other kernel-level test of these kernels runs one pixel (or one 2x2 window) per thread: the grid covers
the tensor, so the grid-stride loop, its U-unrolled body, the hand-over to the tail and the capped grid are
held only by the whole-model step tests (loss 1e-4, logits 5e-3 over millions of pixels: a few wrong pixels do
not show). Each case here first asserts on the host that its size is in the regime it claims (the launchers'
grid rules restated from the exported queries and the constants below), then compares with the references and
bounds the one-pass tests already use (tests/test_gpu_bn_sign.py, tests/test_gpu_kernels.py). Every figure is
printed as a line "coverage: ..." (collected in profiles/pointwise_coverage.txt).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from tests.test_gpu_apply_fused import check_dy_fp64, coefs
from tests.test_gpu_kernels import (bn_fold, check_bnb_sums, check_signed_inputs, gen, kernel_option,  # noqa: F401
                                    nchw, nhwc, rel)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DTYPES = [torch.float32, BF]

# The launch constants csrc/pointwise.hip does not export (line numbers of that file)
TPB = 256               # :39   constexpr int TPB
HU = 4                  # :938  constexpr int HU (pixels per lane group and iteration of the heads kernels)
APPLY_GRID = 1024       # :2004 option(SELUNET_OPT_APPLY_GRID, 1024), selunet_bn_bwd_apply_amax
POOL_FWD_CAP = 8192     # :2045 grid_for(nv, 8192), selunet_maxpool2_fwd
HEADS_FWD_CAP = 8192    # :2085 grid_for(m * 16, 8192), selunet_heads_fwd; :2255 selunet_heads_fwd_planes
APPLY_HEADS_CAP = 2048  # :2117 grid_for(m * 16 / HU, 2048), selunet_bn_bwd_apply_heads;
#                         :2292 grid_for(m * 16, 2048), selunet_bn_bwd_apply_heads_planes
APPLY_U = {0: 4, 1: 8, 2: 8, 3: 16}  # SELUNET_OPT_APPLY_U8 form -> pixels in flight (:589, :2019, :2008, :2012)


def cdiv(a, b):
    return -(-a // b)


def note(what, err, bound):
    print(f"coverage: {what}: {float(err):.2e} (bound {bound:.1e})")


# ------------------------------------------------------------------ the launchers' grid rules, restated
def apply_plan(m, c, form, gcap):
    """(pixel lanes per workgroup, workgroups, pixels in flight) of selunet_bn_bwd_apply_amax (:2001-2026)."""
    pl = TPB // (c // (4 if form >= 2 else 8))
    return pl, max(1, min(cdiv(m, pl), gcap)), APPLY_U[form]


def heads_stride(work_items, cap):
    """Pixels between two iterations of a 16-lanes-per-pixel kernel launched with grid_for(work_items, cap)."""
    return max(1, min(cdiv(work_items, TPB), cap)) * (TPB // 16)


def pool_nv(n, h, w, c):
    return n * (h // 2) * (w // 2) * (c // 4)


APPLY_M = 12293
HEADS_M = 4 * 131072 + 77
PLANES_IMGS, PLANES_HW = 3, 87401
APPLY_HEADS_STRIDE = APPLY_HEADS_CAP * (TPB // 16)
APPLY_HEADS_MS = [2 * APPLY_HEADS_STRIDE + 65, 8 * APPLY_HEADS_STRIDE + 77]
APPLY_HEADS_REGIMES = {APPLY_HEADS_MS[0]: (False, 16353, 189), APPLY_HEADS_MS[1]: (True, 65536, 77)}
APPLY_PLANES_IMGS, APPLY_PLANES_HW = 3, 21867
POOL_BWD_SHAPES = [(3, 64, 64, 512), (3, 150, 148, 64)]
POOL_FWD_SHAPE = (1, 258, 258, 512)


def regime_apply(form, c, gcap):
    pl, grid, u = apply_plan(APPLY_M, c, form, gcap)
    stride = grid * pl
    assert grid == gcap                              # the cap binds
    assert APPLY_M > (u - 1) * stride                # the unrolled loop runs
    full = (APPLY_M - 1 - (u - 1) * stride) // (u * stride) + 1  # its iterations for pixel 0's lane
    assert full >= 2                                 # ... more than once
    rest = APPLY_M - full * u * stride               # pixels left to the tail loop
    assert 0 < rest and rest % stride != 0           # which runs, for a part of the lanes only
    return stride


def regime_heads_fwd():
    stride = heads_stride(HEADS_M * 16, HEADS_FWD_CAP)
    assert stride == HEADS_FWD_CAP * 16 == 131072    # the cap binds
    assert HEADS_M > (HU - 1) * stride               # the unrolled loop runs (for the first 77 pixel groups)
    assert 0 < HEADS_M - HU * stride < stride        # ... once, then the tail takes one pixel for those groups
    return stride


def regime_heads_planes():
    m = PLANES_IMGS * PLANES_HW
    stride = heads_stride(m * 16, HEADS_FWD_CAP)
    assert stride == 131072 and 0 < m - 2 * stride == 59 and PLANES_HW % 2 == 1  # a third pass for 59 pixel groups
    return m


def regime_apply_heads(m):
    """(the cap binds, passes of the HU-unrolled loop over all lane groups, passes of the tail loop), by walking
    the kernel's two loops. The launcher sizes the grid for HU pixels per lane group, so its cap binds from
    m = 4 * 32768 on: just above twice the capped stride the grid still grows with m, most lane groups take the
    unrolled loop once and the last ones three tail passes."""
    stride = heads_stride(m * 16 // HU, APPLY_HEADS_CAP)
    unrolled = tail = 0
    for p in range(stride):
        while p + (HU - 1) * stride < m:
            p, unrolled = p + HU * stride, unrolled + 1
        while p < m:
            p, tail = p + stride, tail + 1
    assert HU * unrolled + tail == m
    return stride == APPLY_HEADS_STRIDE, unrolled, tail


def regime_apply_planes():
    m = APPLY_PLANES_IMGS * APPLY_PLANES_HW
    stride = heads_stride(m * 16, APPLY_HEADS_CAP)
    assert stride == APPLY_HEADS_STRIDE and 0 < m - 2 * stride < stride
    return m


def regime_pool_bwd(n, h, w, c):
    nv = pool_nv(n, h, w, c)
    rows = K.query("selunet_maxpool2_bwd_slab_rows", n, h, w, c)
    assert rows == 1024 and rows * TPB < nv < 2 * rows * TPB  # some threads take a second window, the others one
    return nv, rows


def regime_pool_fwd():
    nv = pool_nv(*POOL_FWD_SHAPE)
    assert nv == 2130048 and nv - POOL_FWD_CAP * TPB == 32896  # threads that wrap
    return nv


# ------------------------------------------------------------------ BN-backward apply under a small grid
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c", [64, 128, 256, 512])
@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_apply_small_grid(form, c, dt, kernel_option):
    """selunet_bn_bwd_apply_amax with SELUNET_OPT_APPLY_GRID = 3 (the unrolled loop runs many times and ends in a
    ragged tail, in every form and at every C) and = 1 (one workgroup does everything): dy against fp64
    (check_dy_fp64, signed fold), and dy and the range word bit-identical to the default grid's."""
    m = APPLY_M
    code = K.dtype_code(dt)
    y = gen(m, c, seed=41).to(dt).to(DEV)
    dz = (gen(m, c, seed=42) * 1e-2).to(dt).to(DEV)
    bn = coefs(c, 50, signed=True)
    sc, sh, mean, invstd, coef = bn
    check_signed_inputs(sc, torch.relu(y.float() * sc + sh))
    kernel_option(("APPLY_U8", form))
    kernel_option(("APPLY_GRID", -1))
    res = []
    for gcap in (None, 3, 1):
        if gcap is not None:
            regime_apply(form, c, gcap)
            K.set_option("APPLY_GRID", gcap)
            assert K.set_option("APPLY_GRID", gcap) == gcap  # the option reads back
        dy = torch.full((m, c), float("nan"), dtype=dt, device=DEV)
        am = torch.zeros(1, device=DEV)
        K.call("selunet_bn_bwd_apply_amax", K.ptr(dz), K.ptr(y), m, c, K.ptr(sc), K.ptr(sh), K.ptr(mean),
               K.ptr(invstd), K.ptr(coef), K.ptr(dy), K.ptr(am), code, K.stream_ptr())
        torch.cuda.synchronize()
        res.append((dy.float().cpu(), am.item()))
    assert not torch.isnan(res[1][0]).any()
    check_dy_fp64(res[1][0], res[1][1], dz, y, bn, dt)
    for dy, am in res[1:]:
        assert torch.equal(dy, res[0][0]) and am == res[0][1]


# ------------------------------------------------------------------ heads forward
@functools.lru_cache(maxsize=2)
def heads_inputs(m, seed, nk):
    """y [m][64] fp32, a signed fold, nk heads (tests/test_gpu_bn_sign.heads_inputs at another m)."""
    y = gen(m, 64, seed=seed)
    s, t = bn_fold(64, seed + 1, signed=True)
    wt, b = gen(nk, 64, seed=seed + 3) * 0.2, gen(nk, seed=seed + 4)
    return y, s, t, wt, b


def heads_ref(y, s, t, wt, b):
    z = torch.relu(y.double() * s.double() + t.double())
    check_signed_inputs(s, z)
    return z @ wt.double().T + b.double()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nh", [1, 3])
def test_heads_fwd_unrolled_and_capped(dt, nh):
    """selunet_heads_fwd at m = 4 * 131072 + 77: the grid is capped, the HU-unrolled loop runs for the first 77
    pixel groups (then one tail pixel) and the tail loop four times for the others. Against relu(y*s + t) @ w.T + b
    in fp64, test_heads_fwd_signed's bound (1e-6 of the output's maximum); no NaN of the pre-fill survives."""
    regime_heads_fwd()
    m = HEADS_M
    y, s, t, wt, b = heads_inputs(m, 230, 3)
    wt, b = wt[:nh], b[:nh]
    y = y.to(dt)
    ref = heads_ref(y, s, t, wt, b)
    yd, sd, td, wd, bd = (x.to(DEV).contiguous() for x in (y, s, t, wt, b))
    outs = [torch.full((m,), float("nan"), device=DEV) for _ in range(nh)]
    K.call("selunet_heads_fwd", K.ptr(yd), m, K.ptr(sd), K.ptr(td), K.ptr(wd), K.ptr(bd), nh,
           *[K.ptr(outs[i]) if i < nh else None for i in range(3)], K.dtype_code(dt), K.stream_ptr())
    torch.cuda.synchronize()
    got = torch.stack(outs, 1).double().cpu()
    assert not torch.isnan(got).any()
    err = float((got - ref).abs().max() / ref.abs().max())
    note(f"heads_fwd nh={nh} {dt}", err, 1e-6)
    assert err < 1e-6


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nk", [3, 8])
def test_heads_fwd_planes_wraps(dt, nk):
    """selunet_heads_fwd_planes at m = 3 x 87401 (odd hw): a third pass for 59 pixel groups, image boundaries at
    pixels that are no multiple of anything; reference and bound of test_heads_fwd_planes_signed."""
    m = regime_heads_planes()
    n_img, hw = PLANES_IMGS, PLANES_HW
    y, s, t, wt, b = heads_inputs(m, 240, 8)
    wt, b = wt[:nk], b[:nk]
    y = y.to(dt)
    ref = heads_ref(y, s, t, wt, b)
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
    err = float((got - ref).abs().max() / ref.abs().max())
    note(f"heads_fwd_planes nk={nk} {dt}", err, 1e-6)
    assert err < 1e-6


# ------------------------------------------------------------------ BN-backward apply forming the heads' dA
def heads_da(w, g, dt):
    """dA [m][64] = sum_k g_k[m] w_k[c] in fp64, rounded to the activation dtype as the producer stores it
    (tests/test_gpu_bn_sign.heads_da)."""
    da = sum(gk.double().cpu()[:, None] * w[k].double().cpu()[None, :] for k, gk in enumerate(g))
    return da.float().to(dt).double()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nh", [1, 3])
@pytest.mark.parametrize("m", APPLY_HEADS_MS)
def test_apply_heads_wraps(m, nh, dt):
    """selunet_bn_bwd_apply_heads just above twice its capped stride (the grid is not capped yet there: one pass of
    the HU-unrolled loop for most lane groups, three tail passes for the last 63) and at 8 x 32768 + 77 (capped:
    the unrolled loop twice for every lane group, then a tail pass for 77): reference and bound of
    test_apply_heads_signed (check_dy_fp64 on the fp64 dA)."""
    assert regime_apply_heads(m) == APPLY_HEADS_REGIMES[m]
    code = K.dtype_code(dt)
    y = gen(m, 64, seed=1).to(dt).to(DEV)
    bn = coefs(64, 10, signed=True)
    sc, sh, mean, invstd, coef = bn
    check_signed_inputs(sc, torch.relu(y.float() * sc + sh))
    w = (gen(3, 64, seed=2) * 0.2).to(DEV).contiguous()
    g = [(gen(m, seed=3 + i) * 1e-3).to(DEV) for i in range(3)]
    gp = [K.ptr(g[i]) if i < nh else None for i in range(3)]
    dy = torch.full((m, 64), float("nan"), dtype=dt, device=DEV)
    am = torch.zeros(1, device=DEV)
    K.call("selunet_bn_bwd_apply_heads", K.ptr(y), m, K.ptr(sc), K.ptr(sh), K.ptr(mean), K.ptr(invstd), K.ptr(coef),
           K.ptr(w), nh, *gp, K.ptr(dy), K.ptr(am), code, K.stream_ptr())
    torch.cuda.synchronize()
    assert not torch.isnan(dy.float()).any()
    check_dy_fp64(dy.float().cpu(), am.item(), heads_da(w, g[:nh], dt), y, bn, dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_apply_heads_planes_wraps(dt):
    """selunet_bn_bwd_apply_heads_planes (6 planes of three [N, 2, hw] gradients, 3 images of odd hw) just above
    twice its capped stride: reference and bound of test_apply_heads_planes_signed."""
    m = regime_apply_planes()
    n, hw, nk = APPLY_PLANES_IMGS, APPLY_PLANES_HW, 6
    code = K.dtype_code(dt)
    y = gen(m, 64, seed=81).to(dt).to(DEV)
    bn = coefs(64, 90, signed=True)
    sc, sh, mean, invstd, coef = bn
    check_signed_inputs(sc, torch.relu(y.float() * sc + sh))
    w = (gen(8, 64, seed=82) * 0.2).to(DEV).contiguous()
    g = (gen(3, n, 2, hw, seed=83) * 1e-3).to(DEV).contiguous()
    hp = K.HeadPlanes()
    hp.n, hp.hw = nk, hw
    for k in range(nk):
        t, j = divmod(k, 2)
        hp.plane[k] = g[t].data_ptr() + j * hw * 4
        hp.img_stride[k] = 2 * hw
        hp.w_off[k], hp.b_off[k] = k * 65, k * 65 + 64
    hp.row_len = nk * 65
    dy = torch.full((m, 64), float("nan"), dtype=dt, device=DEV)
    am = torch.zeros(1, device=DEV)
    K.call("selunet_bn_bwd_apply_heads_planes", K.ptr(y), m, K.ptr(sc), K.ptr(sh), K.ptr(mean), K.ptr(invstd),
           K.ptr(coef), K.ptr(w), hp, K.ptr(dy), K.ptr(am), code, K.stream_ptr())
    torch.cuda.synchronize()
    assert not torch.isnan(dy.float()).any()
    gk = g.reshape(3, n, 2, hw).permute(0, 2, 1, 3).reshape(nk, m)
    check_dy_fp64(dy.float().cpu(), am.item(), heads_da(w[:nk], list(gk), dt), y, bn, dt)


# ------------------------------------------------------------------ max-pool
@functools.lru_cache(maxsize=2)
def pool_case(n, h, w, c):
    """test_maxpool_ties_and_backward's inputs at another shape: duplicated maxima in every window, all-dead
    windows in channels [0, 8); the unit fold makes the argmax exact in any arithmetic. bf16: the inputs are
    rounded first (rounding keeps the ties and the dead windows)."""
    y = gen(n, c, h, w, seed=17)
    y[:, :, ::2, 1::2] = y[:, :, ::2, ::2]
    y[:, :8] = -1.0
    dp = gen(n, c, h // 2, w // 2, seed=18)
    dskip = gen(n, c, h, w, seed=19)
    return y, dp, dskip


def pool_ref(y, dp, dskip):
    z = torch.relu(y).requires_grad_()
    p = F.max_pool2d(z, 2)
    (gz,) = torch.autograd.grad(p, z, dp)
    return p.detach(), gz + dskip


def bnb_err(slab, da, y, scale, shift, mean, invstd):
    """The figure check_bnb_sums asserts on (tests/test_gpu_kernels.py), for the record."""
    y64, da64 = y.double(), da.double()
    g = da64 * (y64 * scale.double() + shift.double() > 0).double()
    xh = (y64 - mean.double()) * invstd.double()
    want = torch.stack([g.sum(0), (g * xh).sum(0), xh.sum(0)])
    got = slab.double().sum(0)
    return float(((got - want).abs() / (want.abs().max(dim=1, keepdim=True).values + 1.0)).max())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,h,w,c", POOL_BWD_SHAPES)
def test_maxpool_bwd_second_window(n, h, w, c, dt):
    """selunet_maxpool2_bwd (storing; storing with the BN-backward sums; sums only with the range word) and
    selunet_bn_bwd_apply_pool with 1024 workgroups and more windows than threads: a part of the threads takes a
    second window and carries its sums and maximum across the iterations. Unit fold, no window left out.
    fp32: dz bit-equal to torch's max_pool2d routing + dskip; bf16: test_maxpool_signed_transform's bound
    (1e-6 + 2^-8 of the maximum). Sums: check_bnb_sums at 1e-5 / 1e-4. The word: max |dz| as stored."""
    nv, rows = regime_pool_bwd(n, h, w, c)
    if c == 64:
        assert nv % (rows * TPB) % TPB != 0  # the second pass ends inside a workgroup
    code = K.dtype_code(dt)
    y, dp, dskip = (t.to(dt).float() for t in pool_case(n, h, w, c))
    _, gz = pool_ref(y, dp, dskip)
    want = nhwc(gz)
    d = lambda t_: nhwc(t_).to(dt).to(DEV).contiguous()  # noqa: E731
    yd, dpd, dsd = d(y), d(dp), d(dskip)
    sd, td = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    mean, invstd = (gen(c, seed=40) * 0.1).to(DEV), (gen(c, seed=41).abs() + 0.5).to(DEV)
    tol = 0.0 if dt == torch.float32 else 1e-6 + 2.0 ** -8
    sum_tol = 1e-5 if dt == torch.float32 else 1e-4
    m = n * h * w
    stored = None
    slabs = []
    for mode in ("store", "store+bnb", "sums"):
        dz = None if mode == "sums" else torch.full((m, c), float("nan"), dtype=dt, device=DEV)
        slab = torch.full((rows, 3, c), float("nan"), device=DEV)
        word = torch.zeros(1, device=DEV)
        bnb = None
        if mode != "store":
            bnb = K.BnBwdStats(K.ptr(yd), K.ptr(sd), K.ptr(td), K.ptr(mean), K.ptr(invstd), K.ptr(slab),
                               K.ptr(word) if mode == "sums" else None)
        K.call("selunet_maxpool2_bwd", K.ptr(yd), n, h, w, c, K.ptr(sd), K.ptr(td), K.ptr(dpd), K.ptr(dsd), K.ptr(dz),
               bnb, code, K.stream_ptr())
        torch.cuda.synchronize()
        if dz is not None:
            got = dz.float().cpu()
            assert not torch.isnan(got).any()
            if dt == torch.float32:
                assert torch.equal(got, want)
            else:
                err = float((got.double() - want.double()).abs().max() / want.double().abs().max())
                note(f"maxpool2_bwd dz {mode} C={c} bf16", err, tol)
                assert err < tol
            assert stored is None or torch.equal(got, stored)
            stored = got
        if bnb is not None:
            args = (slab.cpu(), stored, yd.float().cpu(), sd.cpu(), td.cpu(), mean.cpu(), invstd.cpu())
            note(f"maxpool2_bwd sums {mode} C={c} {dt}", bnb_err(*args), sum_tol)
            check_bnb_sums(*args, tol=sum_tol)
            slabs.append(slab.cpu())
        if mode == "sums":
            assert word.item() == stored.abs().max().item() > 0
    assert torch.equal(slabs[0], slabs[1])
    # the fused apply forms the same dA again (rounded to dt as stored) and applies the BN backward to it
    bn = (sd, td, mean, invstd, (gen(3, c, seed=54) * 0.5).to(DEV).contiguous())
    dy = torch.full((m, c), float("nan"), dtype=dt, device=DEV)
    am = torch.zeros(1, device=DEV)
    K.call("selunet_bn_bwd_apply_pool", K.ptr(yd), n, h, w, c, K.ptr(sd), K.ptr(td), K.ptr(mean), K.ptr(invstd),
           K.ptr(bn[4]), K.ptr(dpd), K.ptr(dsd), K.ptr(dy), K.ptr(am), code, K.stream_ptr())
    torch.cuda.synchronize()
    assert not torch.isnan(dy.float()).any()
    check_dy_fp64(dy.float().cpu(), am.item(), want.to(dt).double(), yd, bn, dt)


@functools.lru_cache(maxsize=1)
def pool_fwd_case():
    n, h, w, c = POOL_FWD_SHAPE
    y = gen(n, c, h, w, seed=117)
    y[:, :, ::2, 1::2] = y[:, :, ::2, ::2]
    y[:, :8] = -1.0
    return y


@pytest.mark.parametrize("dt", DTYPES)
def test_maxpool_fwd_wraps(dt):
    """selunet_maxpool2_fwd at 1 x 258 x 258 x 512: the grid is capped at 8192 workgroups and 32896 threads take a
    second window. Unit fold: bit-equal to F.max_pool2d(relu(y)) (bf16: of the rounded y; a maximum of bf16
    values is a bf16 value)."""
    regime_pool_fwd()
    n, h, w, c = POOL_FWD_SHAPE
    y = pool_fwd_case().to(dt).float()
    want = nhwc(F.max_pool2d(torch.relu(y), 2))
    yd = nhwc(y).to(dt).to(DEV).contiguous()
    sd, td = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    out = torch.full((n * h * w // 4, c), float("nan"), dtype=dt, device=DEV)
    K.call("selunet_maxpool2_fwd", K.ptr(yd), n, h, w, c, K.ptr(sd), K.ptr(td), K.ptr(out), K.dtype_code(dt),
           K.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out.float().cpu(), want)
