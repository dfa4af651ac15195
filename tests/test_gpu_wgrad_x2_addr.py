"""Staging addresses and predicates of the split-fp16 3x3 weight gradient (conv3x3_wgrad_x2_kernel: per-thread
offsets and edge bits formed once, a scalar base and an edge mask per tile).

Every tensor the kernel reads (dY or dA, y, both halo sources, skip, pooled, the heads' planes) is a view carved
from the middle of a NaN-filled allocation with at least (W + 2) C elements on each side, and the outputs (the
weight gradient, dy) are pre-filled with NaN: an out-of-image slot that is staged, a stale clamp or a missed
store shows up as NaN (all inside allocated memory), an indexing mistake as an O(1) error against the fp64
weight gradient at the split-fp16 tolerance. dy and max |dy| of the fused forms must equal the standalone applies
bit for bit.

Shapes: one tile row per image with image boundaries on both sides of the middle image (3 x 8x16), an
interior / edge mix (2 x 16x24), ragged in both directions (12x20, 9x17), a two-tile row that wraps to the next
image (2 x 32x16). The entry points take grids of h >= 8, w >= 16 only (test_entry_point_refuses_8_wide), so
the 8-wide grids 3 x 8x8 and 2 x 32x8 (one tile per image / per tile row) cannot reach the kernel; 8x16 and
32x16 are the narrowest that do: every tile of 8x16 touches the top and bottom edges and one of left / right.
Channel plans cin -> cout: 64 -> 64 (64 columns, both tap groups), 64 + 64 -> 64 (two sources, two channel
chunks), 128 -> 256 (two column tiles, two chunks), 256 -> 128 (four chunks, all of them storing dy)."""
import ctypes
import functools

import pytest
import torch

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from tests.test_gpu_kernels import bn_fold, gen, nhwc, rel
from tests.test_gpu_x2 import TOL, word

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

SHAPES = [(3, 8, 16), (2, 16, 24), (1, 12, 20), (1, 9, 17), (2, 32, 16)]
EVEN = [s for s in SHAPES if s[1] % 2 == 0 and s[2] % 2 == 0]
PLANS = [(64, 0, 64), (64, 64, 64), (128, 0, 256), (256, 0, 128)]  # cin0, cin1, cout


def guarded(t, w, c):
    """t on the device as a view from the middle of a NaN-filled allocation: (W + 2) C elements (rounded to
    16 bytes) of NaN on each side. Returns (view, whole allocation)."""
    pad = ((w + 2) * c + 3) // 4 * 4
    buf = torch.full((2 * pad + t.numel(),), NAN, device=DEV)
    v = buf[pad:pad + t.numel()].view(t.shape)
    v.copy_(t)
    return v, buf


def bands_intact(buf, v):
    pad = (buf.numel() - v.numel()) // 2
    return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + v.numel():]).all())


@functools.lru_cache(maxsize=None)
def halo_operand(cin0, cin1, n, h, w):
    """The 3x3 operand: one or two BN+ReLU sources (the 128-channel plan: one plain source), guarded on the
    device; its fp64 value [N, C, H, W] on the host."""
    xform = cin0 != 128
    keep, srcs, words, parts = [], [], [], []
    for i, c in enumerate([cin0, cin1]):
        if not c:
            words.append(None)
            continue
        x = gen(n, c, h, w, seed=9 + i) * (1e-3 if i else 1.0)  # sources of different ranges
        s, t = bn_fold(c, 20 + 2 * i)
        a = torch.relu(x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)) if xform else x
        xv, xb = guarded(nhwc(x), w, c)
        sd, td = s.to(DEV), t.to(DEV)
        keep += [xb, sd, td]
        srcs.append(K.source(xv, c, sd if xform else None, td if xform else None))
        words.append(word(a.abs().max()))
        parts.append(a.double())
    return K.gather(n, h, w, 9, *srcs), words, torch.cat(parts, 1), keep


def wgrad_ref(a64, g_nhwc, n, h, w):
    """fp64 weight gradient of the [M, cout] gradient g against the operand a64."""
    co = g_nhwc.shape[1]
    g = g_nhwc.double().cpu().reshape(n, h, w, co).permute(0, 3, 1, 2)
    return torch.nn.grad.conv2d_weight(a64, (co, a64.shape[1], 3, 3), g, padding=1)


def workspace(gp, gq):
    wsb = K.query("selunet_conv3x3_wgrad_x2_ws_bytes", gp, gq)
    assert wsb > 0
    return torch.full((wsb // 4,), NAN, device=DEV), wsb


@pytest.fixture
def tile_queue():
    prev = K.set_option("TILE_QUEUE", 0)
    yield lambda v: K.set_option("TILE_QUEUE", v)
    K.set_option("TILE_QUEUE", prev)


def test_entry_point_refuses_8_wide():
    """Grids narrower than 16 do not reach the kernel (the split-fp16 weight gradient shares the halo weight
    gradients' eligibility rule: h >= 8, w >= 16)."""
    for n, h, w in [(3, 8, 8), (2, 32, 8)]:
        x = torch.zeros(n * h * w, 64, device=DEV)
        gp, gq = K.gather(n, h, w, 1, K.source(x, 64)), K.gather(n, h, w, 9, K.source(x, 64))
        assert K.query("selunet_conv3x3_wgrad_x2_ws_bytes", gp, gq) < 0


def run_plain(plan, shape):
    (cin0, cin1, cout), (n, h, w) = plan, shape
    gq, xw, a64, _keep = halo_operand(cin0, cin1, n, h, w)
    dy = nhwc(gen(n, cout, h, w, seed=12) * 1e-9)
    dyv, dyb = guarded(dy, w, cout)
    gp = K.gather(n, h, w, 1, K.source(dyv, cout))
    ws, wsb = workspace(gp, gq)
    outs = []
    for _ in range(2):
        out = torch.full((cout, cin0 + cin1, 3, 3), NAN, device=DEV)
        K.call("selunet_conv3x3_wgrad_x2", gp, gq, K.ptr(ws), wsb, K.ptr(out), K.ptr(word(dy.abs().max())),
               K.ptr(xw[0]), K.ptr(xw[1]), K.stream_ptr())
        outs.append(out)
    torch.cuda.synchronize()
    return outs, wgrad_ref(a64, dy, n, h, w)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("plan", PLANS)
def test_plain(plan, shape):
    outs, ref = run_plain(plan, shape)
    assert bool(torch.isfinite(outs[0]).all())
    e = rel(outs[0], ref)
    print(f"wgrad rel err {e:.2e}")
    assert e < TOL
    assert torch.equal(outs[0], outs[1])  # the static walk is bit-reproducible


def bn_state(m, c, seed):
    y = gen(m, c, seed=seed)
    sc, sh = bn_fold(c, seed + 1)
    mean, invstd = gen(c, seed=seed + 3) * 0.1, gen(c, seed=seed + 4).abs() + 0.5
    coef = gen(3, c, seed=seed + 5) * 0.5
    coef[0] = coef[0].abs() + 0.5
    return y, [t.to(DEV).contiguous() for t in (sc, sh, mean, invstd, coef)]


def run_fused(plan, shape):
    """selunet_conv3x3_wgrad_x2_bn against selunet_bn_bwd_apply_amax: (dy, max |dy|, weight gradients of two
    launches), (the apply's dy, max |dy|), the fp64 weight gradient of the apply's dy."""
    (cin0, cin1, cout), (n, h, w) = plan, shape
    m = n * h * w
    gq, xw, a64, _keep = halo_operand(cin0, cin1, n, h, w)
    y, (sc, sh, mean, invstd, coef) = bn_state(m, cout, 40)
    da = gen(m, cout, seed=47) * 1e-3
    yv, yb = guarded(y, w, cout)
    dav, dab = guarded(da, w, cout)
    dy0 = torch.full((m, cout), NAN, device=DEV)
    am0 = torch.zeros(1, device=DEV)
    K.call("selunet_bn_bwd_apply_amax", K.ptr(dav), K.ptr(yv), m, cout, K.ptr(sc), K.ptr(sh), K.ptr(mean),
           K.ptr(invstd), K.ptr(coef), K.ptr(dy0), K.ptr(am0), K.F32, K.stream_ptr())
    torch.cuda.synchronize()
    gp = K.gather(n, h, w, 1, K.source(dav, cout))
    ws, wsb = workspace(gp, gq)
    bnb = K.BnBwdStats(K.ptr(yv), K.ptr(sc), K.ptr(sh), K.ptr(mean), K.ptr(invstd), None)
    res = []
    for _ in range(2):
        dyv, dyb = guarded(torch.full((m, cout), NAN), w, cout)
        am = torch.zeros(1, device=DEV)
        out = torch.full((cout, cin0 + cin1, 3, 3), NAN, device=DEV)
        K.call("selunet_conv3x3_wgrad_x2_bn", gp, gq, K.ptr(ws), wsb, K.ptr(out), K.ptr(am0), K.ptr(xw[0]),
               K.ptr(xw[1]), bnb, K.ptr(coef), K.ptr(dyv), K.ptr(am), K.stream_ptr())
        torch.cuda.synchronize()
        assert bands_intact(dyb, dyv)
        res.append((dyv, am.item(), out))
    return res, (dy0, am0.item()), wgrad_ref(a64, dy0, n, h, w)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("plan", PLANS)
def test_fused_apply(plan, shape):
    res, (dy0, am0), ref = run_fused(plan, shape)
    for dy, am, out in res:
        assert torch.equal(dy, dy0)
        assert am == am0
        assert bool(torch.isfinite(out).all())
    e = rel(res[0][2], ref)
    print(f"wgrad rel err {e:.2e}")
    assert e < TOL
    assert torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize("shape", EVEN)
@pytest.mark.parametrize("plan", [p for p in PLANS if p[2] == 64])
@pytest.mark.parametrize("form", ["pool", "pool_noskip", "heads1", "heads3"])
def test_fused_sources(form, plan, shape):
    """selunet_conv3x3_wgrad_x2_bn_src with a pool / heads dA source against selunet_bn_bwd_apply_pool / _heads."""
    (cin0, cin1, c), (n, h, w) = plan, shape
    m = n * h * w
    gq, xw, a64, _keep = halo_operand(cin0, cin1, n, h, w)
    y = (gen(m, c, seed=60) * 2).round() / 2  # coarse: ties inside the pool windows
    _, (sc, sh, mean, invstd, coef) = bn_state(m, c, 61)
    yv, yb = guarded(y, w, c)
    dy0 = torch.full((m, c), NAN, device=DEV)
    am0 = torch.zeros(1, device=DEV)
    keep = []
    if form.startswith("pool"):
        dpv, dpb = guarded(gen(m // 4, c, seed=62) * 1e-2, w, c)
        dsv, dsb = guarded(gen(m, c, seed=63) * 1e-2, w, c) if form == "pool" else (None, None)
        keep += [dpb, dsb]
        src = K.DaSource(K.DA_POOL, 0, K.ptr(dpv), K.ptr(dsv))
        K.call("selunet_bn_bwd_apply_pool", K.ptr(yv), n, h, w, c, K.ptr(sc), K.ptr(sh), K.ptr(mean), K.ptr(invstd),
               K.ptr(coef), K.ptr(dpv), K.ptr(dsv), K.ptr(dy0), K.ptr(am0), K.F32, K.stream_ptr())
    else:
        nh = int(form[-1])
        wt = (gen(3, 64, seed=64) * 0.2).to(DEV).contiguous()
        g = [guarded(gen(m, seed=65 + i) * 1e-3, w, 1) for i in range(3)]
        gptr = [K.ptr(g[i][0]) if i < nh else None for i in range(3)]
        keep += [wt, g]
        src = K.DaSource(K.DA_HEADS, nh, None, None, K.ptr(wt), (ctypes.c_void_p * 3)(*gptr))
        K.call("selunet_bn_bwd_apply_heads", K.ptr(yv), m, K.ptr(sc), K.ptr(sh), K.ptr(mean), K.ptr(invstd),
               K.ptr(coef), K.ptr(wt), nh, *gptr, K.ptr(dy0), K.ptr(am0), K.F32, K.stream_ptr())
    torch.cuda.synchronize()
    gp = K.gather(n, h, w, 1, K.source(yv, c))  # grid and channel count only
    ws, wsb = workspace(gp, gq)
    bnb = K.BnBwdStats(K.ptr(yv), K.ptr(sc), K.ptr(sh), K.ptr(mean), K.ptr(invstd), None)
    dyv, dyb = guarded(torch.full((m, c), NAN), w, c)
    am = torch.zeros(1, device=DEV)
    out = torch.full((c, cin0 + cin1, 3, 3), NAN, device=DEV)
    K.call("selunet_conv3x3_wgrad_x2_bn_src", gp, gq, K.ptr(ws), wsb, K.ptr(out), K.ptr(am0), K.ptr(xw[0]),
           K.ptr(xw[1]), bnb, K.ptr(coef), src, K.ptr(dyv), K.ptr(am), K.stream_ptr())
    torch.cuda.synchronize()
    assert bands_intact(dyb, dyv)
    assert torch.equal(dyv, dy0)
    assert am.item() == am0.item()
    assert bool(torch.isfinite(out).all())
    e = rel(out, wgrad_ref(a64, dy0, n, h, w))
    print(f"wgrad rel err {e:.2e}")
    assert e < TOL


@pytest.mark.parametrize("shape", [(2, 16, 24), (1, 12, 20)])
@pytest.mark.parametrize("plan", [(128, 0, 256), (256, 0, 128), (64, 64, 64)])
def test_tile_queue(plan, shape, tile_queue):
    """SELUNET_OPT_TILE_QUEUE = 2 (tiles from ticket counters): the plain and the fused weight gradients within
    the tolerance, dy and max |dy| unchanged."""
    tile_queue(2)
    outs, ref = run_plain(plan, shape)
    assert rel(outs[0], ref) < TOL and rel(outs[1], ref) < TOL
    res, (dy0, am0), ref = run_fused(plan, shape)
    for dy, am, out in res:
        assert torch.equal(dy, dy0) and am == am0
        assert rel(out, ref) < TOL
