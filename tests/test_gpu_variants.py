"""Kernel instantiations and split plans that only an option or an unusual shape selects, through the case
helpers of the default-path tests (the same fp64 / fp32 CPU references and the same tolerances):

* the three 3x3 weight gradients (fp32 halo, fp32 Winograd, bf16 halo) with several pixel tiles per workgroup:
  `wgrad_geom` gives every split `per = cdiv(total, min(total, cdiv(WGRAD_WGS, groups)))` tiles, and at the
  default target of 256 workgroups every kernel-level shape has per == 1, so the walk from one tile to the next
  (double-buffered LDS hand-over, prefetch of the next tile, ragged last split) runs only under a small
  SELUNET_OPT_WGRAD_WGS. Each case restates its plan on the host and asserts it before the launch;
* the fp32 Winograd weight gradient's four instantiations (tile width 16 / 8, 12 / 8 waves);
* the fp32 halo weight gradient on split partials (odd widths, or WINO_WGRAD = 0) with its fixed-order reduction;
* the gather GEMM on halo-sized 3x3 operands (HALO = 0);
* the rejection of more than 64 (co tile, ci chunk) groups by the split-fp16 weight gradient's tile queue.

The non-persistent multi-chunk halo kernel (HALO_PERSIST = 0) is a variant parameter in test_gpu_kernels.py.
tests/test_dispatch_ledger.py names, per kernel, the test here or there that runs it."""
import types

import pytest
import torch

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from tests import test_gpu_kernels as KT
from tests import test_gpu_wino as WI
from tests.test_gpu_kernels import gather_wgs, halo_wgs, kernel_option  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cdiv(a, b):
    return -(-a // b)


def wgrad_plan(kind, n, h, w, cout, cins, wgs=-1, tw=16):
    """The launch plan of a 3x3 weight gradient, restated from conv3x3.hip's wgrad_geom (as test_cabi._splits):
    kind "f32" (fp32 halo: 8x8 pixel tiles), "wino" (fp32 Winograd: 8 x tw tiles, 64-column tiles) or "bf16"
    (bf16 halo: 8x16 tiles); wgs: SELUNET_OPT_WGRAD_WGS (-1: the default, 256). Checked against the workspace
    query and the kernel-name query under the options in force, so call it after they are set."""
    cin = sum(cins)
    bi = 64 if kind == "wino" or cout % 128 else 128
    tile_w = {"f32": 8, "wino": tw, "bf16": 16}[kind]
    groups = (cout // bi) * (cin // 64)
    total = n * cdiv(h, 8) * cdiv(w, tile_w)
    want = max(1, cdiv(max(1, 256 if wgs < 0 else wgs), groups))
    per = cdiv(total, min(total, want))
    splits = cdiv(total, per)
    row = 12 * cin if kind == "wino" else K.query("selunet_wgrad_ld", 9 * cin)
    code = K.BF16 if kind == "bf16" else K.F32
    fake = torch.empty(64)  # never dereferenced: the queries look at shapes only
    gp = K.gather(n, h, w, 1, K.source(fake, cout))
    gq = K.gather(n, h, w, 9, *[K.source(fake, c) for c in cins])
    name = {"f32": f"conv3x3_wgrad_halo_f32<{bi}>", "wino": "conv3x3_wgrad_wino_f32<64>",
            "bf16": f"conv3x3_wgrad_halo<{bi}>"}[kind]
    assert K.query("selunet_gemm_kernel_name", gp, gq, 0, 0, code).decode() == name
    ws_bytes = K.query("selunet_gemm_wgrad_ws_bytes", gp, gq, code)
    assert ws_bytes == splits * cout * row * 4 > 0, (ws_bytes, splits, cout, row)
    return types.SimpleNamespace(groups=groups, total=total, per=per, splits=splits, last=total - (splits - 1) * per)


def assert_walk(plan, walk, min_groups=1):
    """ragged: several splits of several tiles each, the last one shorter; one: a single workgroup per group
    walks every tile (at least four)."""
    if walk == "ragged":
        assert plan.splits >= 2 and plan.per >= 2 and plan.total % plan.per != 0, vars(plan)
        assert 0 < plan.last < plan.per, vars(plan)
    else:
        assert walk == "one" and plan.splits == 1 and plan.per == plan.total >= 4, vars(plan)
    assert plan.groups >= min_groups, vars(plan)


# ------------------------------------------------------------------ weight gradients at per >= 2
# (kind, the case helper's arguments, signed, WGRAD_WGS, walk, least (co tile, ci chunk) groups).
# f32: KT.conv3x3_wgrad_case(cin0, cin1, cout, xform, small, h, w), n = 2, even widths under WINO_WGRAD = 0;
# wino: WI.wino_wgrad_case(cin0, cin1, cout, xform, n, h, w); bf16: KT.conv3x3_bf16_fwd_wgrad_case(cin0, cin1,
# cout, small, h, w), n = 2. Shapes are those of the default-path tests.
PER_CASES = [
    ("f32", (64, 0, 64, True, False, 20, 36), False, 4, "ragged", 1),       # 30 tiles: 8, 8, 8, 6
    ("f32", (64, 0, 64, True, False, 20, 36), True, 4, "ragged", 1),
    ("f32", (64, 0, 64, True, False, 20, 36), False, 1, "one", 1),          # one workgroup, 30 tiles
    ("f32", (128, 0, 256, False, False, 16, 16), False, 12, "ragged", 4),   # BI = 128, 4 groups, 8 tiles: 3, 3, 2
    ("f32", (64, 64, 128, True, False, 16, 16), True, 6, "ragged", 2),      # two sources: 3, 3, 2
    ("wino", (128, 0, 256, False, 1, 20, 36), False, 16, "ragged", 8),      # 9 tiles in 8 groups: 5, 4
    ("wino", (128, 0, 256, False, 1, 20, 36), False, 8, "one", 8),          # one workgroup per group, 9 tiles
    ("wino", (64, 0, 64, True, 2, 20, 36), True, 4, "ragged", 1),           # 18 tiles: 5, 5, 5, 3
    ("wino", (256, 0, 64, True, 3, 12, 18), False, 4, "one", 4),            # 12 tiles
    ("bf16", (128, 0, 64, False, 20, 40), False, 8, "ragged", 2),           # 18 tiles in 2 groups: 5, 5, 5, 3
    ("bf16", (64, 0, 64, False, 20, 40), True, 4, "ragged", 1),
    ("bf16", (128, 0, 64, False, 20, 40), False, 2, "one", 2),              # 18 tiles
    ("bf16", (256, 0, 512, False, 16, 16), False, 16, "one", 16),           # BI = 128, 16 groups, 4 tiles each
    ("bf16", (64, 128, 64, False, 24, 17), False, 3, "one", 3),             # two sources, odd width: 12 tiles
]


def run_wgrad_case(kind, args, signed):
    if kind == "f32":
        KT.conv3x3_wgrad_case(*args, signed=signed)
    elif kind == "wino":
        WI.wino_wgrad_case(*args, signed=signed)
    else:
        KT.conv3x3_bf16_fwd_wgrad_case(*args, signed=signed)


def case_geometry(kind, args):
    """(n, h, w, cout, source channels) of a case helper's arguments."""
    cin0, cin1, cout = args[:3]
    n = args[4] if kind == "wino" else 2
    h, w = args[-2:]
    return n, h, w, cout, [cin0, cin1] if cin1 else [cin0]


@pytest.mark.parametrize("kind,args,signed,wgs,walk,min_groups", PER_CASES)
def test_wgrad_tiles_per_workgroup(kind, args, signed, wgs, walk, min_groups, kernel_option):
    """The three 3x3 weight gradients with per >= 2 pixel tiles per workgroup (see the module docstring): the plan
    is asserted on the host, then the default-path case helper runs under it (fp64 / fp32 conv2d weight gradient,
    the helper's tolerance, selunet_gemm_wgrad_ws against _ws_to bit for bit where the helper asserts that)."""
    kernel_option(("WGRAD_WGS", wgs))
    if kind == "f32":
        kernel_option(("WINO_WGRAD", 0))
    n, h, w, cout, cins = case_geometry(kind, args)
    assert K.set_option("WGRAD_WGS", wgs) == wgs
    assert_walk(wgrad_plan(kind, n, h, w, cout, cins, wgs), walk, min_groups)
    run_wgrad_case(kind, args, signed)


# ------------------------------------------------------------------ Winograd weight-gradient instantiations
WINO_WGRAD_SHAPES = [
    (64, 0, 64, True, 2, 16, 16),       # the shapes of test_wino_wgrad ...
    (64, 64, 128, True, 2, 16, 16),
    (128, 0, 256, False, 1, 20, 36),
    (256, 0, 64, True, 3, 12, 18),
    (64, 64, 64, True, 3, 8, 16),       # ... exactly one 16-wide tile (two 8-wide), one tile row
    (128, 0, 64, True, 2, 10, 22),      # ragged for both tile widths: 16 + 6, 8 + 8 + 6
]


def set_wino_variant(kernel_option, tw, nw, wgs):
    for name, v in (("WINO_WGRAD_TW", tw), ("WINO_WGRAD_WAVES", nw), ("WGRAD_WGS", wgs)):
        kernel_option((name, v))
        assert K.set_option(name, v) == v  # the kernel name carries neither: the options read back


@pytest.mark.parametrize("cin0,cin1,cout,xform,n,h,w", WINO_WGRAD_SHAPES)
@pytest.mark.parametrize("wgs", [-1, 16])
@pytest.mark.parametrize("nw", [12, 8])
@pytest.mark.parametrize("tw", [16, 8])
def test_wino_wgrad_variants(cin0, cin1, cout, xform, n, h, w, tw, nw, wgs, kernel_option):
    """conv3x3_wgrad_wino_f32_kernel<TW, NW> for TW in {16, 8} and NW in {12, 8} (test_wino_wgrad runs <16, 12>
    alone), at the default workgroup target and at 16 (128 -> 256 at 20x36: 5 + 4 tiles at TW = 16, 8 + 7 at
    TW = 8). The workspace query follows cdiv(w, tw) (asserted in wgrad_plan)."""
    set_wino_variant(kernel_option, tw, nw, wgs)
    plan = wgrad_plan("wino", n, h, w, cout, [cin0, cin1] if cin1 else [cin0], wgs, tw)
    assert plan.total == n * cdiv(h, 8) * cdiv(w, tw)
    if (cin0, cout, h, w, wgs) == (128, 256, 20, 36, 16):
        assert (plan.per, plan.last) == ((5, 4) if tw == 16 else (8, 7))
    WI.wino_wgrad_case(cin0, cin1, cout, xform, n, h, w)


# ------------------------------------------------------------------ fp32 halo weight gradient on split partials
# (cin0, cin1, cout, xform, h, w, signed, WGRAD_WGS, WINO_WGRAD): odd widths go to the halo kernel whatever
# WINO_WGRAD says; the even widths only with it off. n = 2.
HALO_F32_WS_CASES = [
    (128, 0, 256, False, 9, 17, False, -1, -1),    # BI = 128, one source
    (128, 0, 256, True, 9, 17, True, -1, -1),
    (64, 64, 64, True, 12, 19, False, -1, -1),     # BI = 64, two BN+ReLU sources
    (64, 64, 64, True, 12, 19, True, -1, -1),
    (128, 0, 256, True, 9, 37, False, 12, -1),     # 20 tiles in 4 groups: 7, 7, 6
    (64, 64, 64, True, 9, 37, True, 6, -1),        # 20 tiles in 2 groups: 7, 7, 6
    (128, 0, 256, False, 9, 18, False, -1, 0),     # the same at even widths, Winograd off
    (64, 64, 64, True, 12, 20, True, -1, 0),
    (128, 0, 256, True, 10, 36, False, 12, 0),     # 20 tiles in 4 groups: 7, 7, 6
]


@pytest.mark.parametrize("cin0,cin1,cout,xform,h,w,signed,wgs,wino", HALO_F32_WS_CASES)
def test_conv3x3_wgrad_halo_f32_split_partials(cin0, cin1, cout, xform, h, w, signed, wgs, wino, kernel_option):
    """conv3x3_wgrad_halo_f32_kernel<128, 64> / <64, 32> writing split partials (ws != NULL) and their fixed-order
    reduction: what the exact-fp32 configuration runs for a layer whose width is odd (a 64x136 patch's 8x17
    level). KT.conv3x3_wgrad_case goes through selunet_gemm_wgrad (atomics), selunet_gemm_wgrad_ws and
    selunet_gemm_wgrad_ws_to (Conv2d layout, pre-filled with NaN), each against torch's weight gradient."""
    kernel_option(("WGRAD_WGS", wgs))
    kernel_option(("WINO_WGRAD", wino))
    assert w % 2 == 1 or wino == 0
    plan = wgrad_plan("f32", 2, h, w, cout, [cin0, cin1] if cin1 else [cin0], wgs)
    if wgs > 0:
        assert_walk(plan, "ragged", 4 if cout == 256 else 2)
    KT.conv3x3_wgrad_case(cin0, cin1, cout, xform, False, h, w, signed=signed)


# ------------------------------------------------------------------ gather GEMM on halo-sized 3x3 operands
@pytest.mark.parametrize("dtype", [K.F32, K.BF16])
def test_gather_gemm_on_halo_sized_3x3(dtype, kernel_option):
    """HALO = 0 (SELUNET_NO_HALO=1): the 3x3 forward with two sources and BN+ReLU at 16x24 and a SPLIT data
    gradient on gemm_gather<T> (otherwise run at 8x8 and 8x12 only). The statistics rows come from
    selunet_gemm_stats_rows, which the helpers query after the option is set."""
    variant = ("HALO", 0)
    kernel_option(variant)
    KT.check_halo_variant(variant, 2, 16, 24, [64, 64], 128, 0, dtype)
    KT.check_halo_variant(variant, 2, 16, 24, [64], 128, 64, dtype)
    if dtype == K.F32:
        KT.conv3x3_fwd_stats_case(64, 64, 128, 2, 16, 24, True)
        KT.conv3x3_dgrad_case(128, 64, 64, 16, 24)
        KT.conv3x3_dgrad_case(64, 64, 0, 16, 24)   # PLAIN with the BN-backward sums
    else:
        KT.conv3x3_bf16_persist_fwd_stats_case(64, 64, 128, 2, 16, 24)
        KT.conv3x3_bf16_persist_dgrad_case(128, 64, 64, 16, 24)
        KT.conv3x3_bf16_persist_dgrad_case(64, 64, 0, 16, 24)


# ------------------------------------------------------------------ option-induced rejections
def test_x2_wgrad_tile_queue_rejects_more_than_64_groups(kernel_option):
    """SELUNET_OPT_TILE_QUEUE bit 1 with more than 64 (co tile, ci chunk) groups: the counters hold 64, so the
    launch is refused on the host (ELAUNCH with a message) before anything is enqueued; the output keeps its
    fill. 1024 x 576 channels: 8 x 9 = 72 groups."""
    n, h, w, cout, cin = 1, 8, 16, 1024, 576
    assert (cout // 128) * (cin // 64) > 64
    p = torch.zeros(n * h * w, cout, device=DEV)
    q = torch.zeros(n * h * w, cin, device=DEV)
    am = torch.ones(1, device=DEV)
    gp, gq = K.gather(n, h, w, 1, K.source(p, cout)), K.gather(n, h, w, 9, K.source(q, cin))
    kernel_option(("TILE_QUEUE", 2))
    wsb = K.query("selunet_conv3x3_wgrad_x2_ws_bytes", gp, gq)
    ws = torch.empty(wsb // 4, device=DEV)
    out = torch.full((cout, cin, 3, 3), 7.0, device=DEV)
    L = K.load()
    rc = L.selunet_conv3x3_wgrad_x2(gp, gq, K.ptr(ws), wsb, K.ptr(out), K.ptr(am), K.ptr(am), None, K.stream_ptr())
    assert rc == 2 and b"64" in L.selunet_last_error()  # SELUNET_ELAUNCH
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
