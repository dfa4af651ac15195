"""Staging addresses of the split-fp16 3x3 convolution (selunet_conv3x3_x2: conv3x3_halo_persist_kernel
<float, BN, X2> static and tile-queue walks, conv3x3_x2d_kernel), which are formed once per thread as 32-bit
offsets from a per-tile scalar base with out-of-image halo slots redirected to the tile's first pixel.

Every source tensor and the packed weights sit inside a larger allocation whose bands (at least one image row
before and after) hold NaN: a load outside the tensor that reaches an accumulator makes the output NaN. Every
output (y / the SPLIT pair, the statistics, BN-backward and column-sum slabs, the range word) sits between bands
of a sentinel bit pattern that must come back unchanged.

References and bounds: y against F.conv2d in fp64 with the tolerance of tests/test_gpu_x2.py (TOL); the BN
statistics (with and without stats_center), the column sums and the BN-backward sums against fp64 sums of the
kernel's own output with the bounds tests/test_gpu_bn_shift.py (stat_tol(fp32_run)), test_x2_dgrad (1e-6) and
check_bnb_sums use for these kernels; the range word equals the exact max |stored value|. The static walk and
the tile queue give bit-identical y and range word, and a repeated call is bit-identical in everything.

Shapes: the smallest at which each address path can go wrong (h, w >= 16, cin % 32 == 0 and cin > 32 are
entry-point limits), each under workgroup counts 0 (default) and 3 (a workgroup walks several tiles, crosses
image boundaries and takes the deferred first-chunk path), conv3x3_x2d on and off where cout == 64, the tile
queue off and on, and a first source with BN+ReLU coefficients, without coefficients (raw values, with exact
-0.0f among them) and with coefficients but relu = 0. Epilogues per mode: PLAIN with BN statistics (with and
without stats_center), PLAIN with BN-backward sums, SPLIT with column sums at split = 64 and 128 where the entry
point takes it (0 < split < cout: none at cout = 64, only 64 at cout = 128).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from tests.test_gpu_bn_shift import check_shifted_sums, fp32_run, stat_tol
from tests.test_gpu_kernels import bn_fold, check_bnb_sums, gen, nchw, nhwc, rel
from tests.test_gpu_x2 import SLACKS, TOL, pack_x2

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5A5AC3C3  # bit pattern of the output bands (a finite float: 1.5e16)

SHAPES = [
    (64, 0, 64, 2, 16, 16),      # one tile per image, every edge at once, image boundary between consecutive tiles
    (64, 0, 128, 1, 18, 35),     # ragged in both directions, odd width
    (128, 0, 256, 2, 20, 24),    # two column tiles, ragged rows
    (64, 64, 128, 1, 16, 48),    # two sources with different ranges, BN = 128
    (128, 128, 64, 1, 32, 16),   # two sources, BN = 64 (M16)
    (64, 0, 64, 3, 33, 17),      # one ragged pixel row and column, three images
    (512, 0, 128, 1, 16, 16),    # sixteen chunks, one tile
]
SOURCES = ("bnrelu", "raw", "bn_norelu")


def banded_in(t, band):
    """t (fp32) inside an allocation whose bands of `band` elements hold NaN; the view keeps 16-B alignment."""
    band = (band + 63) // 64 * 64
    buf = torch.full((t.numel() + 2 * band,), float("nan"), device=DEV)
    view = buf[band:band + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


class Out:
    """An fp32 output between two sentinel bands (the tensor itself starts as `fill`)."""

    def __init__(self, shape, fill=float("nan"), band=1024):
        n = 1
        for s in shape:
            n *= s
        self.band, self.n = band, n
        self.buf = torch.empty(n + 2 * band, device=DEV)
        self.buf.view(torch.int32).fill_(SENTINEL)
        self.t = self.buf[band:band + n].view(shape)
        self.t.fill_(fill)

    def check(self):
        bits = self.buf.view(torch.int32)
        assert bool((bits[:self.band] == SENTINEL).all()) and bool((bits[self.band + self.n:] == SENTINEL).all())
        assert not torch.isnan(self.t).any()
        return self.t


@functools.lru_cache(maxsize=None)
def case(cin0, cin1, cout, n, h, w, source):
    """Inputs, fp64 reference and range words of one case (read-only, shared between the modes)."""
    x0 = gen(n, cin0, h, w, seed=1)
    x1 = gen(n, cin1, h, w, seed=2) * 1e-3 if cin1 else None  # sources of different ranges
    wt = gen(cout, cin0 + cin1, 3, 3, seed=3, scale=0.05)
    s0, t0 = bn_fold(cin0, 10)
    if source == "raw":
        x0.view(-1)[::7] = -0.0  # exact negative zeros, at image corners and edges among them
        a0 = x0
    elif source == "bnrelu":
        a0 = torch.relu(x0 * s0.view(1, -1, 1, 1) + t0.view(1, -1, 1, 1))
    else:
        a0 = x0 * s0.view(1, -1, 1, 1) + t0.view(1, -1, 1, 1)
    a, s1, t1, a1 = a0, None, None, None
    if cin1:
        s1, t1 = bn_fold(cin1, 12)
        a1 = torch.relu(x1 * s1.view(1, -1, 1, 1) + t1.view(1, -1, 1, 1))
        a = torch.cat((a0, a1), 1)
    ref = F.conv2d(a.double(), wt.double(), padding=1)
    r = ref.permute(1, 0, 2, 3).reshape(cout, -1)
    center = (r.mean(1) + 0.3 * r.std(1, unbiased=False)).float()
    return dict(x0=x0, x1=x1, wt=wt, s0=s0, t0=t0, s1=s1, t1=t1, ref=ref, center=center,
                am0=float(a0.abs().max()) * 1.5, am1=float(a1.abs().max()) if cin1 else None)


def modes(cout):
    """(workgroups, x2d, tile queue): the tile queue only matters where conv3x3_x2d does not take the layer."""
    for wgs in (0, 3):
        for x2d in ((1, 0) if cout == 64 else (0,)):
            for tq in ((0,) if x2d else (0, 1)):
                yield wgs, x2d, tq


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("cin0,cin1,cout,n,h,w", SHAPES)
def test_x2_conv_staging_addresses(cin0, cin1, cout, n, h, w, source):
    staging_case(cin0, cin1, cout, n, h, w, source)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("cin0,cin1,cout,n,h,w", [SHAPES[0], SHAPES[3]])
def test_x2_conv_staging_addresses_loose_words(cin0, cin1, cout, n, h, w, slack):
    """Both input range words multiplied by `slack` (as training's Samuelson bounds are above the real maximum):
    same checks, same bounds."""
    staging_case(cin0, cin1, cout, n, h, w, "bnrelu", slack=slack)


def staging_case(cin0, cin1, cout, n, h, w, source, slack=1.0):
    c = case(cin0, cin1, cout, n, h, w, source)
    M = n * h * w
    assert K.query("selunet_conv3x3_x2_ok", h, w, cin0 + cin1, cin0, cout) == 1
    coef = source != "raw"
    keep = []  # K.source holds raw pointers: the allocations stay alive here

    def banded(t, band):
        v, buf = banded_in(t.to(DEV).contiguous(), band)
        keep.append(buf)
        return v

    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    sc_keep = [d(c["s0"]), d(c["t0"])]
    srcs = [K.source(banded(nhwc(c["x0"]), w * cin0), cin0, sc_keep[0] if coef else None, sc_keep[1] if coef else None,
                     relu=source == "bnrelu")]
    am0, am1 = torch.tensor([c["am0"] * slack], device=DEV), None
    if cin1:
        sc_keep += [d(c["s1"]), d(c["t1"])]
        srcs.append(K.source(banded(nhwc(c["x1"]), w * cin1), cin1, sc_keep[2], sc_keep[3]))
        am1 = torch.tensor([c["am1"] * slack], device=DEV)
    u0, _ = pack_x2(c["wt"], dgrad=False)
    u = banded(u0, w * (cin0 + cin1))
    g = K.gather(n, h, w, 9, *srcs)
    ptiles = n * -(-h // 16) * -(-w // 16)
    # operands of the BN-backward sums epilogue (as test_x2_dgrad)
    yprev = gen(M, cout, seed=42).to(DEV)
    bsc, bsh = (gen(cout, seed=43).abs() + 0.5).to(DEV), (gen(cout, seed=44) * 0.3).to(DEV)
    mean, invstd = (gen(cout, seed=45) * 0.1).to(DEV), (gen(cout, seed=46).abs() + 0.5).to(DEV)
    center = c["center"].to(DEV)
    # (the SPLIT epilogue needs 0 < split < cout)
    epilogues = ["stats", "stats_center", "bnb"] + [f"split{s}" for s in (64, 128) if s < cout]

    def run(kind, rows):
        """One launch: returns (y [M][cout] on the CPU, slab on the CPU or None, range word or None)."""
        word = Out((1,), 0.0)
        if kind in ("stats", "stats_center"):
            y, slab = Out((M, cout)), Out((rows, 2, cout))
            ep = K.Epilogue(K.ptr(y.t), None, None, K.ptr(slab.t), K.EP_PLAIN, 0)
            if kind == "stats_center":
                ep.stats_center = K.ptr(center)
            outs = [y, slab]
        elif kind == "bnb":
            y, slab = Out((M, cout)), Out((rows, 3, cout))
            ep = K.Epilogue(K.ptr(y.t), None, None, None, K.EP_PLAIN, 0)
            ep.bnb = K.BnBwdStats(K.ptr(yprev), K.ptr(bsc), K.ptr(bsh), K.ptr(mean), K.ptr(invstd), K.ptr(slab.t))
            ep.amax = K.ptr(word.t)
            outs = [y, slab, word]
        else:
            split = int(kind[5:])
            y, y1, slab = Out((M, split)), Out((M, cout - split)), Out((rows, split))
            ep = K.Epilogue(K.ptr(y.t), K.ptr(y1.t), None, None, K.EP_SPLIT, split, K.ptr(slab.t))
            ep.amax = K.ptr(word.t)
            outs = [y, slab, word, y1]
        K.call("selunet_conv3x3_x2", g, K.ptr(u), cout, ep, K.ptr(am0), K.ptr(am1), K.stream_ptr())
        torch.cuda.synchronize()
        for o in outs:
            o.check()
        full = torch.cat((y.t, y1.t), 1) if kind.startswith("split") else y.t
        return full.cpu(), slab.t.cpu(), (word.t.item() if word in outs else None), y.t.cpu()

    prev = (K.query("selunet_set_halo_workgroups", 0), K.set_option("X2D", -1), K.set_option("TILE_QUEUE", -1))
    try:
        for wgs, x2d, tq in modes(cout):
            K.query("selunet_set_halo_workgroups", wgs)
            K.set_option("X2D", x2d)
            K.set_option("TILE_QUEUE", tq)
            rows = K.query("selunet_conv3x3_x2_stats_rows", g, cout)
            kernel = K.query("selunet_conv3x3_x2_kernel_name", g, cout, K.EP_PLAIN, 0).decode()
            tol = stat_tol(fp32_run(kernel, ptiles, rows))
            static = {}
            for kind in epilogues:
                y, slab, word, y0 = run(kind, rows)
                err = rel(nchw(y, n, h, w), c["ref"])
                print(f"{kernel} wgs {wgs} tq {tq} {kind}: y error {err:.2e} (bound {TOL:.0e})")
                assert err < TOL, (kernel, wgs, tq, kind)
                if kind == "stats":
                    check_shifted_sums(slab, y, None, tol)
                elif kind == "stats_center":
                    check_shifted_sums(slab, y, center, tol)
                elif kind == "bnb":
                    check_bnb_sums(slab.to(DEV), y.to(DEV), yprev, bsc, bsh, mean, invstd)
                else:
                    assert rel(slab.double().sum(0), y0.double().sum(0)) < 1e-6
                if word is not None:
                    assert word == y.abs().max().item() > 0  # the exact max |stored value|
                again = run(kind, rows)  # a second call: everything bit-identical
                assert torch.equal(again[0], y) and torch.equal(again[1], slab) and again[2] == word
                static[kind] = (y, word)
            if tq == 0 and not x2d:
                walk = static
            elif tq == 1:  # the tile queue against the static walk of the same workgroup count
                for kind in epilogues:
                    assert torch.equal(static[kind][0], walk[kind][0]) and static[kind][1] == walk[kind][1], kind
    finally:
        K.query("selunet_set_halo_workgroups", prev[0])
        K.set_option("X2D", prev[1])
        K.set_option("TILE_QUEUE", prev[2])
