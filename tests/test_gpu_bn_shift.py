"""The shifted BatchNorm statistics path of fp32 training (engine.Engine.bn_shift, on by default), at kernel
level through the C-ABI:

1. every conv kernel family with selunet_epilogue.stats_center set (the slab then holds the sums of v - c and
   (v - c)^2), checked per channel against the fp64 sums over the kernel's own stored output, so the conv
   rounding stays out of the check;
2. the finalize chain as engine._cbr issues it: selunet_bn_stats_finalize_shifted ->
   selunet_bn_centered_partials_adaptive(ratio = +inf) -> selunet_bn_stats_finalize_centered_bound, with the
   center buffer carried from call to call, against the fp64 statistics of y.

bf16 is out of scope: the engine passes a center only in fp32 training (engine._cbr), so no bf16 kernel is run
with one here.

Tolerance of the shifted sums (STAT_TOL = 4e-6, relative to sum |d| resp. sum d^2 of the channel): d = v - c and
d * d round once in fp32, a thread then adds at most its tile's rows in fp32 before it folds them into a double
accumulator (StatAcc<float>; the most is 32 rows, in the first-layer kernel), and the slab row rounds once more:
about 36 * 2^-24 = 2.1e-6 in the worst case, doubled. The kernels that keep their statistics in fp32 for longer
(single-chunk halo kernel, the 128-column split-fp16 and Winograd kernels, conv3x3_x2p) get the same formula with
their own run length, see fp32_run. A center taken from the wrong column or one unmasked row of a partial tile
moves a sum by about M * |delta c| resp. |c|: four or more orders of magnitude above either bound.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from tests.test_gpu_kernels import bn_fold, gen, halo_wgs, kernel_option, nchw, nhwc, pack, rel  # noqa: F401
from tests.test_gpu_wino import pack_wino
from tests.test_gpu_x2 import pack_x2, tile_queue, word, x2d  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
STAT_TOL = 4e-6
CENTERS = ("null", "zeros", "near", "far")


def stat_tol(run):
    """Bound of the shifted sums for a kernel whose longest sequential fp32 accumulation has `run` terms:
    STAT_TOL up to 32, else the same derivation with the kernel's own length, 2 * (run + 4) * 2^-24."""
    return STAT_TOL if run <= 32 else 2.0 * (run + 4) * 2.0 ** -24


def fp32_run(kernel, ptiles, rows):
    """Terms of the longest sequential fp32 sum behind one slab value of `kernel` (read from the kernels'
    epilogues, lds_tile_store_acc / tile_stats_flush with TR = 256 tile pixels): a thread adds its
    TR / (threads / (TC / 8)) rows of a tile in fp32; kernels with fp64 statistics registers fold that into a
    double and reduce the workgroup in fp64 (run = those rows, at most 8). The others stay in fp32:
      conv3x3_halo1<f32,64>  one tile, 512 threads, 64 columns: 4 rows, then 64 row groups summed in fp32;
      conv3x3_x2p<f32,128>   per 32-column quarter, 256 threads: 4 rows, then 64 row groups in fp32 (then fp64);
      conv3x3_halo<f32,64>   (HALO_PERSIST = 0) one tile, fp32 registers, as conv3x3_halo1: 4 rows, then 64 row groups;
      conv3x3_halo<f32,128>  the same with 128 columns: 512 / 16 = 32 row groups of 8 rows each;
      conv3x3_x2<f32,128>, conv3x3_wino<128>  fp32 registers over all tiles of the workgroup (8 rows each,
                             ceil(ptiles / rows) tiles; one with the tile queue, rows == ptiles), then 32 row groups."""
    if kernel in ("conv3x3_halo1<f32,64>", "conv3x3_x2p<f32,128>", "conv3x3_halo<f32,64>"):
        return 4 + 64
    if kernel == "conv3x3_halo<f32,128>":
        return 8 + 32
    if kernel in ("conv3x3_x2<f32,128>", "conv3x3_wino<128>"):
        return 8 * -(-ptiles // rows) + 32
    assert kernel in ("gemm_gather<f32>", "conv3x3_halo_persist<f32,64>", "conv3x3_halo_persist<f32,128>",
                      "conv3x3_x2d<f32,64>", "conv3x3_x2<f32,64>", "conv3x3_wino<64>"), kernel
    return 8


@functools.lru_cache(maxsize=None)
def conv_case(cin0, cin1, cout, n, h, w, x1_scale=1.0):
    """Inputs of one 3x3 conv case (as test_conv3x3_fwd_stats / test_x2_fwd_stats build them), its fp64 CPU
    reference [N][cout][h][w] and the reference's per-channel mean and standard deviation. Shared between the
    parametrisations: read-only."""
    x0 = gen(n, cin0, h, w, seed=1)
    x1 = gen(n, cin1, h, w, seed=2) * x1_scale if cin1 else None
    wt = gen(cout, cin0 + cin1, 3, 3, seed=3, scale=0.05)
    s0, t0 = bn_fold(cin0, 10)
    a0 = torch.relu(x0 * s0.view(1, -1, 1, 1) + t0.view(1, -1, 1, 1))
    a, s1, t1, a1 = a0, None, None, None
    if cin1:
        s1, t1 = bn_fold(cin1, 12)
        a1 = torch.relu(x1 * s1.view(1, -1, 1, 1) + t1.view(1, -1, 1, 1))
        a = torch.cat((a0, a1), 1)
    ref = F.conv2d(a.double(), wt.double(), padding=1)
    r = ref.permute(1, 0, 2, 3).reshape(cout, -1)
    return dict(x0=x0, x1=x1, wt=wt, s0=s0, t0=t0, s1=s1, t1=t1, ref=ref, mu=r.mean(1), sigma=r.std(1, unbiased=False),
                am0=float(a0.abs().max()), am1=float(a1.abs().max()) if cin1 else None)


def make_centers(mu, sigma):
    """The four centers of the issue: NULL, zeros, mu + 0.3 sigma and mu + 3 sigma (fp32, per channel)."""
    return {"null": None, "zeros": torch.zeros(len(mu), device=DEV),
            "near": (mu + 0.3 * sigma).float().to(DEV), "far": (mu + 3.0 * sigma).float().to(DEV)}


def check_shifted_sums(slab, y, c, tol):
    """slab [rows][2][C] against the fp64 sums of d = y - c and d^2 over the kernel's own output y [M][C]."""
    assert not torch.isnan(slab).any()  # every slab row was written
    d = y.double().cpu() - (c.double().cpu() if c is not None else 0.0)
    got = slab.double().cpu().sum(0)
    e1, b1 = (got[0] - d.sum(0)).abs(), d.abs().sum(0)
    e2, b2 = (got[1] - (d * d).sum(0)).abs(), (d * d).sum(0)
    print(f"shifted sums: worst error / bound scale {float((e1 / b1).max()):.2e} (sum d), "
          f"{float((e2 / b2).max()):.2e} (sum d^2), tolerance {tol:.2e}")
    assert (e1 <= tol * b1).all(), (int((e1 / b1).argmax()), float((e1 / b1).max()))
    assert (e2 <= tol * b2).all(), (int((e2 / b2).argmax()), float((e2 / b2).max()))


def check_family(launch, M, cout, rows, case, tol, y_tol):
    """launch(y, stats, center) under the four centers: y bit-identical, zeros == null in the slab, every slab
    against the sums of the kernel's own output shifted by its center."""
    centers = make_centers(case["mu"], case["sigma"])
    outs = {}
    for name in CENTERS:
        y = torch.full((M, cout), float("nan"), device=DEV)
        stats = torch.full((rows, 2, cout), float("nan"), device=DEV)
        launch(y, stats, centers[name])
        torch.cuda.synchronize()
        outs[name] = (y, stats)
    y0, s0 = outs["null"]
    n, _, h, w = case["ref"].shape
    assert rel(nchw(y0.cpu(), n, h, w), case["ref"]) < y_tol
    for name in CENTERS[1:]:
        assert torch.equal(outs[name][0], y0), name  # the shift never touches the stored values
    assert torch.equal(outs["zeros"][1], s0)
    for name in CENTERS:
        check_shifted_sums(outs[name][1], y0, centers[name], tol)


def conv_sources(case, cin0, cin1, with_words):
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    keep = [d(nhwc(case["x0"])), d(case["s0"]), d(case["t0"])]  # K.source holds raw pointers: kept alive by the caller
    srcs = [K.source(keep[0], cin0, keep[1], keep[2])]
    words = [word(case["am0"] * 1.5) if with_words else None, None]
    if cin1:
        keep += [d(nhwc(case["x1"])), d(case["s1"]), d(case["t1"])]
        srcs.append(K.source(keep[3], cin1, keep[4], keep[5]))
        words[1] = word(case["am1"]) if with_words else None
    return keep, srcs, words


@pytest.mark.parametrize("cin0,cin1,cout,n,h,w", [
    (64, 0, 128, 3, 5, 7),       # M = 105: a partial 128-row tile of the gather GEMM
    (256, 256, 256, 1, 4, 4),    # two column tiles
    (64, 0, 64, 2, 32, 32),      # the halo-tile kernel
    (128, 0, 256, 2, 20, 24),    # partial halo tiles, two column tiles
    (32, 0, 64, 2, 24, 20),      # the weights-resident single-chunk kernel
])
@pytest.mark.parametrize("wgs", [0, 3])
def test_gemm_gather_shifted_stats(cin0, cin1, cout, n, h, w, wgs, halo_wgs):
    halo_wgs(wgs)
    gemm_gather_shifted_stats_case(cin0, cin1, cout, n, h, w)


@pytest.mark.parametrize("cin0,cin1,cout,n,h,w,kernel", [
    (64, 0, 64, 2, 32, 32, "conv3x3_halo<f32,64>"),
    (128, 0, 256, 2, 20, 24, "conv3x3_halo<f32,128>"),   # partial halo tiles, two column tiles
])
def test_gemm_gather_shifted_stats_nonpersistent(cin0, cin1, cout, n, h, w, kernel, kernel_option):
    """The shifted statistics epilogue of the non-persistent multi-chunk halo kernel (HALO_PERSIST = 0): one slab
    row per 16x16 tile, summed in fp32 registers over the tile (fp32_run)."""
    kernel_option(("HALO_PERSIST", 0))
    assert gemm_gather_shifted_stats_case(cin0, cin1, cout, n, h, w) == kernel
    # ... and its output range word (ep.amax): the largest |stored value|, one atomic per workgroup
    case = conv_case(cin0, cin1, cout, n, h, w)
    fwd, _, kpad = pack(case["wt"])
    keep, srcs, _ = conv_sources(case, cin0, cin1, False)
    y = torch.full((n * h * w, cout), float("nan"), device=DEV)
    am = torch.zeros(1, device=DEV)
    ep = K.Epilogue(K.ptr(y), None, None, None, K.EP_PLAIN, 0)
    ep.amax = K.ptr(am)
    K.call("selunet_gemm_gather", K.gather(n, h, w, 9, *srcs), K.ptr(fwd), cout, kpad, ep, K.F32, K.stream_ptr())
    torch.cuda.synchronize()
    assert rel(nchw(y.cpu(), n, h, w), case["ref"]) < 1e-4
    assert am.item() == y.abs().max().item()


def gemm_gather_shifted_stats_case(cin0, cin1, cout, n, h, w):
    case = conv_case(cin0, cin1, cout, n, h, w)
    fwd, _, kpad = pack(case["wt"])
    keep, srcs, _ = conv_sources(case, cin0, cin1, False)
    g = K.gather(n, h, w, 9, *srcs)
    rows = K.query("selunet_gemm_stats_rows", g, cout, K.F32)
    kernel = K.query("selunet_gemm_kernel_name", g, None, cout, K.EP_PLAIN, K.F32).decode()
    ptiles = n * -(-h // 16) * -(-w // 16)

    def launch(y, stats, center):
        ep = K.Epilogue(K.ptr(y), None, None, K.ptr(stats), K.EP_PLAIN, 0)
        ep.stats_center = K.ptr(center)
        K.call("selunet_gemm_gather", g, K.ptr(fwd), cout, kpad, ep, K.F32, K.stream_ptr())

    check_family(launch, n * h * w, cout, rows, case, stat_tol(fp32_run(kernel, ptiles, rows)), 1e-4)
    return kernel


@pytest.mark.parametrize("cin0,cin1,cout,n,h,w", [
    (64, 0, 128, 1, 18, 35),     # partial tiles both ways
    (128, 128, 64, 1, 32, 16),   # two sources, 64 columns
    (64, 0, 64, 2, 64, 48),      # several tiles per workgroup
    (128, 0, 256, 2, 20, 24),    # two column tiles; conv3x3_x2p: the column-quarter offset
])
@pytest.mark.parametrize("wgs", [0, 3])
@pytest.mark.parametrize("x2d_mode,tq", [(1, 0), (0, 0), (0, 1), (0, 2)])
def test_x2_shifted_stats(cin0, cin1, cout, n, h, w, wgs, x2d_mode, tq, halo_wgs, x2d, tile_queue):
    halo_wgs(wgs)
    x2d(x2d_mode)
    tile_queue(tq)
    case = conv_case(cin0, cin1, cout, n, h, w, 1e-3)  # sources of different ranges
    assert K.query("selunet_conv3x3_x2_ok", h, w, cin0 + cin1, cin0, cout) == 1
    u, _ = pack_x2(case["wt"], dgrad=False)
    keep, srcs, (am0, am1) = conv_sources(case, cin0, cin1, True)
    g = K.gather(n, h, w, 9, *srcs)
    rows = K.query("selunet_conv3x3_x2_stats_rows", g, cout)
    kernel = K.query("selunet_conv3x3_x2_kernel_name", g, cout, K.EP_PLAIN, 0).decode()
    ptiles = n * -(-h // 16) * -(-w // 16)
    if tq == 1 and kernel.startswith("conv3x3_x2<"):
        assert rows == ptiles  # the tile queue: one slab row per pixel tile

    def launch(y, stats, center):
        ep = K.Epilogue(K.ptr(y), None, None, K.ptr(stats), K.EP_PLAIN, 0)
        ep.stats_center = K.ptr(center)
        K.call("selunet_conv3x3_x2", g, K.ptr(u), cout, ep, K.ptr(am0), K.ptr(am1), K.stream_ptr())

    check_family(launch, n * h * w, cout, rows, case, stat_tol(fp32_run(kernel, ptiles, rows)), 2e-6)


@pytest.mark.parametrize("cin0,cin1,cout,n,h,w", [
    (128, 0, 256, 2, 20, 24),    # partial edge tiles, two 128-column tiles
    (128, 128, 64, 1, 32, 16),   # two sources, 64 columns
])
@pytest.mark.parametrize("wgs", [0, 3])
def test_wino_shifted_stats(cin0, cin1, cout, n, h, w, wgs, halo_wgs):
    halo_wgs(wgs)
    case = conv_case(cin0, cin1, cout, n, h, w)
    assert K.query("selunet_conv3x3_wino_ok", h, w, cin0 + cin1, cin0, cout) == 1
    u, _ = pack_wino(case["wt"], dgrad=False)
    keep, srcs, _ = conv_sources(case, cin0, cin1, False)
    g = K.gather(n, h, w, 9, *srcs)
    rows = K.query("selunet_gemm_stats_rows", g, cout, K.F32)
    kernel = "conv3x3_wino<128>" if cout % 128 == 0 else "conv3x3_wino<64>"  # (conv3x3_wino_bn128, PLAIN epilogue)
    ptiles = n * -(-h // 16) * -(-w // 16)

    def launch(y, stats, center):
        ep = K.Epilogue(K.ptr(y), None, None, K.ptr(stats), K.EP_PLAIN, 0)
        ep.stats_center = K.ptr(center)
        K.call("selunet_conv3x3_wino", g, K.ptr(u), cout, ep, K.stream_ptr())

    check_family(launch, n * h * w, cout, rows, case, stat_tol(fp32_run(kernel, ptiles, rows)), 2e-6)


@pytest.mark.parametrize("cin,n,h,w", [(3, 2, 32, 32), (2, 1, 20, 40)])
def test_first_conv_shifted_stats(cin, n, h, w):
    """selunet_first_conv_fwd_centered: a lane adds its 32 rows of a tile in fp32, its partner half-wave's sum and
    the four waves' (run 36, the case STAT_TOL is derived for); with center NULL it is selunet_first_conv_fwd."""
    x = gen(n, cin, h, w, seed=50)
    wt = gen(64, cin, 3, 3, seed=51, scale=0.2)
    ref = F.conv2d(x.double(), wt.double(), padding=1)
    r = ref.permute(1, 0, 2, 3).reshape(64, -1)
    case = dict(ref=ref, mu=r.mean(1), sigma=r.std(1, unbiased=False))
    xd, wd = x.to(DEV).contiguous(), wt.to(DEV).contiguous()
    fwd = torch.empty(64, 32, device=DEV)
    K.call("selunet_pack_conv3x3", K.ptr(wd), 64, cin, 32, K.ptr(fwd), None, K.F32, K.stream_ptr())
    M = n * h * w
    rows = K.query("selunet_first_conv_rows", n, h, w)

    def launch(y, stats, center):
        K.call("selunet_first_conv_fwd_centered", K.ptr(xd), n, cin, h, w, K.ptr(fwd), K.ptr(y), K.ptr(stats),
               K.ptr(center), K.F32, K.stream_ptr())

    check_family(launch, M, 64, rows, case, STAT_TOL, 1e-4)
    y0, s0 = torch.empty(M, 64, device=DEV), torch.full((rows, 2, 64), float("nan"), device=DEV)
    y1, s1 = torch.empty(M, 64, device=DEV), torch.full((rows, 2, 64), float("nan"), device=DEV)
    K.call("selunet_first_conv_fwd", K.ptr(xd), n, cin, h, w, K.ptr(fwd), K.ptr(y0), K.ptr(s0), K.F32, K.stream_ptr())
    launch(y1, s1, None)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(s0, s1)


def test_center_without_slab_is_rejected():
    n, h, w, c = 1, 16, 16, 64
    x = torch.zeros(n * h * w, c, device=DEV)
    fwd, _, kpad = pack(torch.zeros(64, c, 3, 3))
    y = torch.empty(n * h * w, 64, device=DEV)
    center = torch.zeros(64, device=DEV)
    ep = K.Epilogue(K.ptr(y), None, None, None, K.EP_PLAIN, 0)
    ep.stats_center = K.ptr(center)
    with pytest.raises(K.SelunetError):
        K.call("selunet_gemm_gather", K.gather(n, h, w, 9, K.source(x, c)), K.ptr(fwd), 64, kpad, ep, K.F32,
               K.stream_ptr())
    xi = torch.zeros(n, 3, h, w, device=DEV)
    wp = torch.zeros(64, 32, device=DEV)
    with pytest.raises(K.SelunetError):
        K.call("selunet_first_conv_fwd_centered", K.ptr(xi), n, 3, h, w, K.ptr(wp), K.ptr(y), None, K.ptr(center),
               K.F32, K.stream_ptr())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the finalize chain
M_FIN = 50000
MOMENTUM, EPS = 0.1, 1e-5


def channel_plan(c):
    """Per-channel (mean, std) of test_bn_adaptive_centered_variance (groups of four channels: mean 300 / 0.3 with
    std 1, and near-constant channels, mean 3e-3 with std 3.16e-5) and the groups that get the far center: of the
    groups g % 8 = 0..7 (means 300, 0.3, 300, tiny, 300, 0.3, 300, tiny) the far ones are 2, 3, 5, 6 — half of the
    groups, and both centers for every kind of channel."""
    ch = torch.arange(c)
    means = torch.where(ch % 8 < 4, 300.0, 0.3)
    tiny = ch % 16 >= 12
    means = torch.where(tiny, 3e-3, means)
    stds = torch.where(tiny, 3.16e-5, 1.0)
    far = torch.tensor([(int(g) % 8) in (2, 3, 5, 6) for g in ch // 4])
    return means.double(), stds.double(), far


@functools.lru_cache(maxsize=None)
def fin_batch(c, seed=11, shift=0.0):
    """y [M_FIN][c] fp32 (means moved by `shift` standard deviations) with its fp64 mean and biased / unbiased
    variance. Shared: read-only."""
    means, stds, _ = channel_plan(c)
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(M_FIN, c, generator=g, dtype=torch.float64) * stds + means + shift * stds).float()
    yd = y.double()
    return y, yd.mean(0), yd.var(0, unbiased=False), yd.var(0, unbiased=True)


@functools.lru_cache(maxsize=None)
def bn_params(c):
    """conv bias, gamma (signed, its largest |value| in the last channel: the last block and lane of the
    finalize's range-word maximum), beta and the initial running statistics (running_var on each channel's own
    variance scale, so that its update stays visible in the tiny channels)."""
    _, stds, _ = channel_plan(c)
    bias = gen(c, seed=21) * 0.1
    gamma = gen(c, seed=22)
    gamma = torch.where(gamma.abs() < 0.25, 0.25, gamma)
    gamma[c - 1] = -3.5
    beta = gen(c, seed=23) * 0.5
    rm0 = gen(c, seed=24) * 0.3
    rv0 = ((gen(c, seed=25).abs() + 0.5) * stds ** 2).float()
    return bias, gamma, beta, rm0, rv0


def shifted_slab(y, center, rows):
    """What the conv epilogue hands to the finalize: the sums of (y - c) and (y - c)^2 over `rows` row chunks,
    here exact (fp64) and rounded once to the fp32 slab."""
    d = y.double() - center.double().cpu()
    slab = torch.empty(rows, 2, y.shape[1], dtype=torch.float64)
    for i, ch in enumerate(torch.tensor_split(d, rows)):
        slab[i, 0] = ch.sum(0)
        slab[i, 1] = (ch * ch).sum(0)
    return slab.float().to(DEV)


class Chain:
    """The three launches of engine._cbr's fp32 training statistics on one layer's buffers."""

    def __init__(self, c, with_bound=True):
        self.c = c
        bias, gamma, beta, rm0, rv0 = bn_params(c)
        d = lambda t: t.clone().to(DEV)  # noqa: E731
        self.bias, self.gamma, self.beta, self.rm, self.rv = d(bias), d(gamma), d(beta), d(rm0), d(rv0)
        self.nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        self.center = torch.zeros(c, device=DEV)  # written by the launches only
        self.ws = torch.empty(K.query("selunet_reduce_ws_bytes", 2 * c) // 8, dtype=torch.float64, device=DEV)
        self.bound = torch.zeros(1, device=DEV) if with_bound else None

    def fresh_running(self):
        _, _, _, rm0, rv0 = bn_params(self.c)
        self.rm, self.rv = rm0.clone().to(DEV), rv0.clone().to(DEV)
        self.nbt = torch.zeros((), dtype=torch.int64, device=DEV)

    def step(self, y, rows):
        c, M = self.c, y.shape[0]
        yd = y.to(DEV)
        slab = shifted_slab(y, self.center, rows)
        mean, invstd, scale, shift = (torch.full((c,), float("nan"), device=DEV) for _ in range(4))
        uvar = torch.zeros(c, device=DEV)
        K.call("selunet_bn_stats_finalize_shifted", K.ptr(slab), rows, K.ptr(self.ws), M, c, K.ptr(self.center),
               K.ptr(self.bias), K.ptr(self.gamma), K.ptr(self.beta), 1.0, K.ptr(mean), K.ptr(uvar), K.ptr(invstd),
               K.ptr(scale), K.ptr(shift), K.stream_ptr())
        torch.cuda.synchronize()
        first = dict(mean=mean.clone(), center=self.center.clone(), uvar=uvar.clone())
        rows2 = K.query("selunet_bn_centered_rows", M)
        slab2 = torch.full((rows2, 2, c), float("nan"), device=DEV)
        K.call("selunet_bn_centered_partials_adaptive", K.ptr(yd), M, c, K.ptr(mean), K.ptr(uvar), float("inf"),
               K.ptr(slab2), K.F32, K.stream_ptr())
        K.call("selunet_bn_stats_finalize_centered_bound", K.ptr(slab2), rows2, K.ptr(self.ws), None, M, c,
               K.ptr(mean), K.ptr(self.bias), K.ptr(self.gamma), K.ptr(self.beta), K.ptr(self.rm), K.ptr(self.rv),
               K.ptr(self.nbt), MOMENTUM, EPS, K.ptr(mean), K.ptr(invstd), K.ptr(scale), K.ptr(shift),
               K.ptr(self.bound), K.stream_ptr())
        torch.cuda.synchronize()
        return dict(first=first, slab2=slab2, mean=mean, invstd=invstd, scale=scale, shift=shift, rm=self.rm.clone(),
                    rv=self.rv.clone(), nbt=int(self.nbt), center=self.center.clone())


def check_statistics(r, m64, v64, uv64, rm_prev, rv_prev, bias, sel=slice(None)):
    """Final mean, the variance recovered from invstd and the running variance at the tolerances of
    test_bn_adaptive_centered_variance (1e-6, 1e-5, 2e-5) against the fp64 statistics of y; the running mean within
    1e-6 of its scale. The running buffers start non-trivial, so the 2e-5 applies to the term the launch adds,
    momentum * unbiased variance, plus the one fp32 rounding of the stored sum (2^-23 of it)."""
    mean, invstd = r["mean"].cpu().double()[sel], r["invstd"].cpu().double()[sel]
    m64, v64, uv64 = m64[sel], v64[sel], uv64[sel]
    assert ((mean - m64).abs() / (m64.abs() + 1)).max() < 1e-6
    var = 1.0 / invstd ** 2 - EPS
    assert ((var - v64).abs() / v64.clamp(min=1e-5)).max() < 1e-5
    want_rv = (1 - MOMENTUM) * rv_prev.double()[sel] + MOMENTUM * uv64
    err_rv = (r["rv"].cpu().double()[sel] - want_rv).abs()
    assert (err_rv <= 2e-5 * MOMENTUM * uv64 + 2.0 ** -23 * want_rv).all(), float((err_rv / (MOMENTUM * uv64)).max())
    want_rm = (1 - MOMENTUM) * rm_prev.double()[sel] + MOMENTUM * (m64 + bias.double()[sel])
    assert ((r["rm"].cpu().double()[sel] - want_rm).abs() / (want_rm.abs() + 1)).max() < 1e-6
    # the folded coefficients are those of the final statistics: scale = gamma / sqrt(var + eps) inherits half the
    # variance bound (1e-5 allowed), shift = beta - mean * scale the mean's 1e-6 (|mean| + 1) and the scale's
    gamma, beta = r["gamma"].double()[sel], r["beta"].double()[sel]
    sc = gamma / (v64 + EPS).sqrt()
    assert ((r["scale"].cpu().double()[sel] - sc).abs() / sc.abs()).max() < 1e-5
    sh = beta - m64 * sc
    assert ((r["shift"].cpu().double()[sel] - sh).abs() / (sh.abs() + sc.abs() * (m64.abs() + 1))).max() < 1e-5


@pytest.mark.parametrize("rows", [1, 37, 1025])  # 1025: the two-launch form of the fused reduce + finalize
@pytest.mark.parametrize("c", [64, 256])
def test_finalize_chain_flags_and_statistics(c, rows):
    y, m64, v64, uv64 = fin_batch(c)
    _, _, far = channel_plan(c)
    bias, gamma, beta, rm0, rv0 = bn_params(c)
    sd = v64.sqrt()
    c0 = (m64 + torch.where(far, 3.0, 0.3) * sd).float()  # (mean - c)^2 / var = 9: flagged, 0.09: not
    results = []
    for with_bound in (True, False):
        ch = Chain(c, with_bound)
        ch.center.copy_(c0)
        r = ch.step(y, rows)
        r.update(gamma=gamma, beta=beta, bound=ch.bound)
        results.append(r)
    r = results[0]
    first = r["first"]
    flags = first["uvar"].cpu().double()
    assert torch.equal(flags == -1.0, far)
    assert ((flags[~far] - uv64[~far]).abs() / uv64[~far]).max() < 1e-5
    assert torch.equal(first["center"], first["mean"])  # the next step's center is this step's mean, bit for bit
    assert ((first["mean"].cpu().double() - m64).abs() / (m64.abs() + 1)).max() < 1e-6
    check_statistics(r, m64, v64, uv64, rm0, rv0, bias)
    assert r["nbt"] == 1
    assert torch.equal(r["center"], first["center"])  # the later launches leave it alone
    # no second pass over the unflagged groups: row 0 = (0, (M - 1) * uvar) in fp32, zero rows below
    slab2 = r["slab2"].cpu()
    assert not torch.isnan(slab2).any()
    keep = ~far
    assert torch.equal(slab2[0, 0, keep], torch.zeros(int(keep.sum())))
    assert torch.equal(slab2[0, 1, keep], first["uvar"].cpu()[keep] * torch.tensor(float(M_FIN - 1)))
    assert not slab2[1:, :, keep].any()
    assert (slab2[:, 1, far] > 0).all()  # the flagged groups were re-read by every block
    # the range word of relu(bn(y))
    sq = math.sqrt(M_FIN)
    want = float((gamma.double().abs() * sq + beta.double().abs()).max()) * 1.0001
    got = float(r["bound"].item())
    assert abs(got - want) <= 2e-4 * want
    ab = torch.empty(1, device=DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    K.call("selunet_act_bound", K.ptr(gd), K.ptr(bd), c, M_FIN, K.ptr(ab), K.stream_ptr())
    assert got <= float(ab.item())
    z = torch.relu((y.double() - m64) / (v64 + EPS).sqrt() * gamma.double() + beta.double())
    assert got >= float(z.max())
    # bound = NULL: every other output bit-identical
    r2 = results[1]
    for k in ("mean", "invstd", "scale", "shift", "rm", "rv", "center", "slab2"):
        assert torch.equal(r[k], r2[k]), k
    assert torch.equal(first["uvar"], r2["first"]["uvar"]) and r2["nbt"] == 1


def test_center_carried_over_steps():
    """Four successive batches through one Chain (one center buffer, written by the launches only): the first
    finds the zero center of a recorded step, the means then drift by 0.2 sigma per step (ratio 0.04: no group
    re-read) and jump by 5 sigma at the fourth (ratio 25: every group re-read)."""
    c, rows = 64, 37
    bias, gamma, beta, rm0, rv0 = bn_params(c)
    means, stds, _ = channel_plan(c)
    ch = Chain(c)
    rm_prev, rv_prev = rm0, rv0
    for k, shift in enumerate((0.0, 0.2, 0.4, 5.4)):
        y, m64, v64, uv64 = fin_batch(c, seed=31 + k, shift=shift)
        center_in = ch.center.clone()
        r = ch.step(y, rows)
        r.update(gamma=gamma, beta=beta)
        flags = r["first"]["uvar"].cpu() == -1.0
        if k == 0:  # zero center: flagged where mean^2 > var (means 300 and the near-constant channels)
            assert torch.equal(center_in, torch.zeros(c, device=DEV))
            assert torch.equal(flags, means ** 2 > stds ** 2)
        elif k < 3:
            assert not flags.any(), k
        else:
            assert flags.all()
        if k:
            assert torch.equal(center_in, prev_mean)  # this step ran on the previous step's first-pass mean
        prev_mean = r["first"]["mean"]
        assert torch.equal(r["center"], prev_mean)
        check_statistics(r, m64, v64, uv64, rm_prev, rv_prev, bias)
        assert r["nbt"] == k + 1
        rm_prev, rv_prev = r["rm"].cpu(), r["rv"].cpu()


def test_nonfinite_mean_resets_center():
    """A NaN in one channel's batch: its mean is not carried (center 0, pointwise.hip bn_finalize_one), every
    other center is; the next, finite batch gets correct statistics in every channel from that center."""
    c, rows = 64, 37
    bias, gamma, beta, rm0, rv0 = bn_params(c)
    y, m64, _, _ = fin_batch(c, seed=41)
    y = y.clone()
    y[12345, 7] = float("nan")
    ch = Chain(c)
    r = ch.step(y, rows)
    center = r["center"].cpu()
    assert center[7].item() == 0.0
    others = torch.arange(c) != 7
    assert torch.isfinite(center[others]).all()
    assert torch.equal(center[others], r["first"]["mean"].cpu()[others])
    assert ((center[others].double() - m64[others]).abs() / (m64[others].abs() + 1)).max() < 1e-6
    y2, m2, v2, uv2 = fin_batch(c, seed=42, shift=0.1)
    ch.fresh_running()  # (channel 7's running statistics took the NaN, as torch's would)
    r2 = ch.step(y2, rows)
    r2.update(gamma=gamma, beta=beta)
    assert not (r2["first"]["uvar"].cpu() == -1.0).any()  # 0.1 sigma from the carried means; channel 7: 0.3^2 < 1
    check_statistics(r2, m2, v2, uv2, rm0, rv0, bias)
    assert r2["nbt"] == 1 and torch.isfinite(r2["center"]).all()
