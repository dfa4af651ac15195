"""A ledger of the convolution kernels the dispatch code can pick, without a GPU: for every name the three
kernel-name queries return (selunet_gemm_kernel_name, selunet_conv3x3_x2_kernel_name,
selunet_conv3x3_wino_kernel_name), and for every instantiation that only an option selects without changing the
name, one row saying under which options and for which operand the library picks it and which numerical test
runs it against a CPU reference.

The test asserts that the query answers the row's name under the row's options, that the named test function
exists, and that the ledger's names are exactly the names UNet_B's layers can dispatch to (collected over the
layer list of layout.py at three patch sizes, both dtypes and the kernel-selection options at 0 and 1). A new
kernel name, or a layer moving to a kernel the ledger does not know, fails here until somebody says which
numerical test runs it. SELUNET_OPT_TILE_QUEUE needs a device for its counters: without one the option is
refused and its row is checked for the test function alone (as test_cabi does).

Also pinned here, on the host: an option that makes an operand unrunnable is refused with a message before any
launch (SELUNET_OPT_X2P with a SPLIT epilogue the kernel cannot route, or a scatter epilogue)."""
import ctypes
import importlib
import itertools
import os

import pytest
import torch

import selectivenet_for_semantic_segmentation_binary_amd.layout as L
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import build as B

F32, BF16 = K.F32, K.BF16
PLAIN, SPLIT, SCATTER = K.EP_PLAIN, K.EP_SPLIT, K.EP_SCATTER2X
REFUSED = -(2 ** 63)  # selunet_set_option's answer when an option cannot be set

KN, VT, WN, X2, BS, CT = ("tests.test_gpu_kernels", "tests.test_gpu_variants", "tests.test_gpu_wino",
                          "tests.test_gpu_x2", "tests.test_gpu_bn_sign", "tests.test_gpu_convt_bf16")

# Operands (never dereferenced):
#   ("gather", n, h, w, taps, source channels, BN+ReLU sources, n_cols, epilogue mode)  selunet_gemm_kernel_name, q NULL
#   ("wgrad", n, h, w, P channels, Q taps, Q source channels)                           selunet_gemm_kernel_name, p and q
#   ("x2", n, h, w, source channels, BN+ReLU sources, n_cols, mode, split)              selunet_conv3x3_x2_kernel_name
#   ("wino", n_cols, mode, split)                                                       selunet_conv3x3_wino_kernel_name
# Rows: (options, dtype, operand, kernel name, "module::test function", a UNet_B layer can reach it).
LEDGER = [
    # ---- 3x3 forward / data gradient through selunet_gemm_gather
    ({}, F32, ("gather", 2, 24, 20, 9, (32,), True, 64, PLAIN), "conv3x3_halo1<f32,64>",
     f"{KN}::test_conv3x3_fwd_stats", False),  # 32 fp32 channels: no layer (the first conv has a kernel of its own)
    ({}, BF16, ("gather", 2, 40, 36, 9, (64,), True, 64, PLAIN), "conv3x3_halo1<bf16,64>",
     f"{KN}::test_conv3x3_bf16_persist_fwd_stats", True),
    ({}, F32, ("gather", 2, 20, 24, 9, (128,), True, 256, PLAIN), "conv3x3_halo_persist<f32,128>",
     f"{KN}::test_conv3x3_fwd_stats", True),
    ({}, F32, ("gather", 2, 32, 32, 9, (64,), True, 64, PLAIN), "conv3x3_halo_persist<f32,64>",
     f"{KN}::test_conv3x3_fwd_stats", True),
    ({}, BF16, ("gather", 2, 20, 72, 9, (128,), True, 128, PLAIN), "conv3x3_halo_persist<bf16,128>",
     f"{KN}::test_conv3x3_bf16_persist_fwd_stats", True),
    ({}, BF16, ("gather", 2, 20, 40, 9, (128,), True, 64, PLAIN), "conv3x3_halo_persist<bf16,64>",
     f"{KN}::test_conv3x3_bf16_persist_fwd_stats", True),
    ({"HALO_PERSIST": 0}, F32, ("gather", 2, 20, 24, 9, (128,), True, 256, PLAIN), "conv3x3_halo<f32,128>",
     f"{KN}::test_conv3x3_fwd_stats_variant", True),
    ({"HALO_PERSIST": 0}, F32, ("gather", 2, 32, 32, 9, (64,), False, 128, SPLIT), "conv3x3_halo<f32,64>",
     f"{KN}::test_conv3x3_dgrad_variant", True),
    ({"HALO_PERSIST": 0}, BF16, ("gather", 1, 33, 40, 9, (128, 128), True, 256, PLAIN), "conv3x3_halo<bf16,128>",
     f"{KN}::test_conv3x3_bf16_persist_fwd_stats", True),
    ({"HALO_PERSIST": 0}, BF16, ("gather", 2, 20, 40, 9, (128,), True, 64, PLAIN), "conv3x3_halo<bf16,64>",
     f"{KN}::test_conv3x3_bf16_persist_fwd_stats", True),
    ({}, F32, ("gather", 1, 8, 12, 9, (128,), False, 256, PLAIN), "gemm_gather<f32>",
     f"{KN}::test_conv3x3_fwd_stats", True),
    ({"HALO": 0}, F32, ("gather", 2, 16, 24, 9, (64, 64), True, 128, PLAIN), "gemm_gather<f32>",
     f"{VT}::test_gather_gemm_on_halo_sized_3x3", True),
    ({"HALO": 0}, BF16, ("gather", 2, 16, 24, 9, (64, 64), True, 128, PLAIN), "gemm_gather<bf16>",
     f"{VT}::test_gather_gemm_on_halo_sized_3x3", True),
    # ---- ConvTranspose2d forward / data gradient (bf16; the fp32 forms go through selunet_gemm_gather_x2)
    ({}, BF16, ("gather", 2, 9, 64, 1, (128,), True, 256, SCATTER), "convt<bf16>", f"{CT}::test_convT_bf16_fwd", True),
    ({}, BF16, ("gather", 2, 9, 64, 4, (64,), False, 128, PLAIN), "convt_dgrad<bf16>",
     f"{CT}::test_convT_bf16_dgrad", True),
    # ---- weight gradients
    ({}, F32, ("wgrad", 2, 8, 8, 128, 9, (64,)), "gemm_wgrad<f32>", f"{KN}::test_conv3x3_wgrad", True),
    ({}, BF16, ("wgrad", 2, 4, 6, 256, 4, (128,)), "gemm_wgrad_bf16", f"{KN}::test_convT_bf16_wgrad", True),
    ({}, BF16, ("wgrad", 2, 16, 16, 512, 9, (256,)), "conv3x3_wgrad_halo<128>",
     f"{KN}::test_conv3x3_bf16_fwd_wgrad", True),
    ({}, BF16, ("wgrad", 2, 20, 40, 64, 9, (128,)), "conv3x3_wgrad_halo<64>",
     f"{KN}::test_conv3x3_bf16_fwd_wgrad", True),
    ({"WGRAD_WGS": 8}, BF16, ("wgrad", 2, 20, 40, 64, 9, (128,)), "conv3x3_wgrad_halo<64>",
     f"{VT}::test_wgrad_tiles_per_workgroup", True),
    ({}, F32, ("wgrad", 2, 16, 16, 64, 9, (64,)), "conv3x3_wgrad_wino_f32<64>", f"{WN}::test_wino_wgrad", True),
    ({"WINO_WGRAD_TW": 8, "WINO_WGRAD_WAVES": 12}, F32, ("wgrad", 1, 20, 36, 256, 9, (128,)),
     "conv3x3_wgrad_wino_f32<64>", f"{VT}::test_wino_wgrad_variants", True),
    ({"WINO_WGRAD_TW": 8, "WINO_WGRAD_WAVES": 8}, F32, ("wgrad", 1, 20, 36, 256, 9, (128,)),
     "conv3x3_wgrad_wino_f32<64>", f"{VT}::test_wino_wgrad_variants", True),
    ({"WINO_WGRAD_TW": 16, "WINO_WGRAD_WAVES": 8}, F32, ("wgrad", 1, 20, 36, 256, 9, (128,)),
     "conv3x3_wgrad_wino_f32<64>", f"{VT}::test_wino_wgrad_variants", True),
    ({"WINO_WGRAD_TW": 8, "WINO_WGRAD_WAVES": 8}, F32, ("wgrad", 2, 20, 36, 64, 9, (64,)),
     "conv3x3_wgrad_wino_f32<64>", f"{BS}::test_wino_wgrad_signed_variants", True),
    # (odd width: no Winograd output pairs, so the split-partials entry points run the halo kernel too)
    ({}, F32, ("wgrad", 2, 9, 17, 256, 9, (128,)), "conv3x3_wgrad_halo_f32<128>",
     f"{VT}::test_conv3x3_wgrad_halo_f32_split_partials", True),
    ({}, F32, ("wgrad", 2, 12, 19, 64, 9, (64, 64)), "conv3x3_wgrad_halo_f32<64>",
     f"{VT}::test_conv3x3_wgrad_halo_f32_split_partials", True),
    ({"WINO_WGRAD": 0}, F32, ("wgrad", 2, 9, 18, 256, 9, (128,)), "conv3x3_wgrad_halo_f32<128>",
     f"{VT}::test_conv3x3_wgrad_halo_f32_split_partials", True),
    ({"WINO_WGRAD": 0}, F32, ("wgrad", 2, 12, 20, 64, 9, (64, 64)), "conv3x3_wgrad_halo_f32<64>",
     f"{VT}::test_conv3x3_wgrad_halo_f32_split_partials", True),
    ({"WINO_WGRAD": 0, "WGRAD_WGS": 12}, F32, ("wgrad", 2, 16, 16, 256, 9, (128,)), "conv3x3_wgrad_halo_f32<128>",
     f"{VT}::test_wgrad_tiles_per_workgroup", True),
    # ---- split-fp16 and Winograd 3x3 forward / data gradient
    ({"X2D": 0, "X2P": 0}, F32, ("x2", 2, 20, 24, (128,), True, 256, PLAIN, 0), "conv3x3_x2<f32,128>",
     f"{X2}::test_x2_fwd_stats", True),
    ({"X2D": 0, "X2P": 0, "TILE_QUEUE": 1}, F32, ("x2", 2, 20, 24, (128,), True, 256, PLAIN, 0),
     "conv3x3_x2<f32,128>", f"{X2}::test_x2_fwd_stats", True),
    ({"X2D": 0, "X2P": 0}, F32, ("x2", 2, 16, 16, (64,), True, 64, PLAIN, 0), "conv3x3_x2<f32,64>",
     f"{X2}::test_x2_fwd_stats", True),
    ({"X2D": 1}, F32, ("x2", 2, 16, 16, (64,), True, 64, PLAIN, 0), "conv3x3_x2d<f32,64>",
     f"{X2}::test_x2_fwd_stats", True),
    ({"X2D": 0, "X2P": 1}, F32, ("x2", 2, 20, 24, (128,), True, 256, PLAIN, 0), "conv3x3_x2p<f32,128>",
     f"{X2}::test_x2_fwd_stats", True),
    ({}, F32, ("wino", 256, PLAIN, 0), "conv3x3_wino<f32,128>", f"{WN}::test_wino_fwd_stats", True),
    ({}, F32, ("wino", 128, SPLIT, 64), "conv3x3_wino<f32,64>", f"{WN}::test_wino_dgrad", True),
]

# every name the three queries can return (gemm.hip), "invalid" and "?" (malformed operands) aside
ALL_NAMES = ({f"conv3x3_{k}<{t},{bn}>" for k in ("halo", "halo_persist") for t in ("f32", "bf16") for bn in (64, 128)}
             | {"conv3x3_halo1<f32,64>", "conv3x3_halo1<bf16,64>", "convt<bf16>", "convt_dgrad<bf16>",
                "gemm_gather<f32>", "gemm_gather<bf16>", "gemm_wgrad<f32>", "gemm_wgrad_bf16",
                "conv3x3_wgrad_wino_f32<64>", "conv3x3_wgrad_halo<128>", "conv3x3_wgrad_halo<64>",
                "conv3x3_wgrad_halo_f32<128>", "conv3x3_wgrad_halo_f32<64>", "conv3x3_x2d<f32,64>",
                "conv3x3_x2p<f32,128>", "conv3x3_x2<f32,128>", "conv3x3_x2<f32,64>", "conv3x3_wino<f32,128>",
                "conv3x3_wino<f32,64>"})


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(K.lib_path()):
        B.build()
    return K.load()


class _options:
    """Set options by name for a block (value -1: the default) and put the previous values back. `refused`: an
    option the library could not set (SELUNET_OPT_TILE_QUEUE without a device)."""

    def __init__(self, **kv):
        self.kv = kv
        self.refused = False

    def __enter__(self):
        self.prev = []
        for k, v in self.kv.items():
            p = K.set_option(k, v)
            if p == REFUSED:
                self.refused = True
            else:
                self.prev.append((k, p))
        return self

    def __exit__(self, *exc):
        for k, v in reversed(self.prev):
            K.set_option(k, v)


# the options the ledger's rows and the layer walk set; pinned to their defaults around every row, so that the
# environment's SELUNET_* choices (mapped onto options when the library loads) cannot change an answer
DEFAULTS = dict(HALO=-1, HALO_PERSIST=-1, WINO=-1, WINO_WGRAD=-1, WINO_WGRAD_TW=-1, WINO_WGRAD_WAVES=-1,
                WGRAD_WGS=-1, X2D=-1, X2P=0, TILE_QUEUE=0)

_FAKE = torch.empty(64)  # stands for every data / scale / shift pointer: the queries never dereference them


def _src(c, bn):
    return K.source(_FAKE, c, _FAKE if bn else None, _FAKE if bn else None)


def kernel_name(dtype, operand):
    kind = operand[0]
    if kind == "gather":
        _, n, h, w, taps, cins, bn, n_cols, mode = operand
        g = K.gather(n, h, w, taps, *[_src(c, bn) for c in cins])
        return K.query("selunet_gemm_kernel_name", ctypes.byref(g), None, n_cols, mode, dtype).decode()
    if kind == "wgrad":
        _, n, h, w, cp, taps, cqs = operand
        gp, gq = K.gather(n, h, w, 1, _src(cp, False)), K.gather(n, h, w, taps, *[_src(c, False) for c in cqs])
        return K.query("selunet_gemm_kernel_name", ctypes.byref(gp), ctypes.byref(gq), 0, 0, dtype).decode()
    if kind == "x2":
        _, n, h, w, cins, bn, n_cols, mode, split = operand
        g = K.gather(n, h, w, 9, *[_src(c, bn) for c in cins])
        return K.query("selunet_conv3x3_x2_kernel_name", ctypes.byref(g), n_cols, mode, split).decode()
    _, n_cols, mode, split = operand
    return K.query("selunet_conv3x3_wino_kernel_name", n_cols, mode, split).decode()


@pytest.mark.parametrize("row", range(len(LEDGER)))
def test_ledger_row(row, lib):
    """The library picks the row's kernel for the row's operand under the row's options, the options read back,
    and the test the row names exists."""
    options, dtype, operand, name, test, _ = LEDGER[row]
    module, _, function = test.partition("::")
    assert callable(getattr(importlib.import_module(module), function))
    assert name in ALL_NAMES
    with _options(**DEFAULTS), _options(**options) as o:
        if o.refused:
            assert "TILE_QUEUE" in options and not torch.cuda.is_available()
            return
        for k, v in options.items():
            assert K.set_option(k, v) == v
        assert kernel_name(dtype, operand) == name
        if operand[0] == "wgrad" and name.startswith("conv3x3_wgrad"):
            # the 3x3 weight gradients have a split-partials form: the fixed-order (deterministic) path
            _, n, h, w, cp, taps, cqs = operand
            gp, gq = K.gather(n, h, w, 1, _src(cp, False)), K.gather(n, h, w, taps, *[_src(c, False) for c in cqs])
            assert K.query("selunet_gemm_wgrad_ws_bytes", ctypes.byref(gp), ctypes.byref(gq), dtype) > 0


# spatial divisor of every CBR block's level (three 2x2 max-pools down, three ConvTranspose2d up)
LEVEL = {"encoder_layer_1": 1, "encoder_layer_2": 2, "encoder_layer_3": 4, "decoder_layer_4": 8,
         "decoder_layer_3": 4, "decoder_layer_2": 2, "decoder_layer_1": 1}


def layer_names(n, H, W, dtype):
    """Every kernel name the queries give for UNet_B's 3x3 and ConvTranspose2d layers (forward, data gradient,
    weight gradient) at an n x H x W input, under the options in force. encoder_layer_1_1 (3 input channels) and
    the 1x1 heads have entry points of their own and no name query."""
    names = set()
    gemm = lambda g, q, n_cols, mode: names.add(  # noqa: E731
        K.query("selunet_gemm_kernel_name", ctypes.byref(g), ctypes.byref(q) if q else None, n_cols, mode,
                dtype).decode())
    for name, ci, co in L.CBR_LAYERS:
        if ci is None:
            continue
        d = LEVEL[name[:-2]]
        h, w = H // d, W // d
        cat = name.startswith("decoder") and name.endswith("_2") and LEVEL[name[:-2]] != 8  # torch.cat(up, skip)
        cins = (ci // 2, ci // 2) if cat else (ci,)
        mode, split = (SPLIT, ci // 2) if cat else (PLAIN, 0)
        fwd = K.gather(n, h, w, 9, *[_src(c, True) for c in cins])
        dgr = K.gather(n, h, w, 9, _src(co, False))
        gemm(fwd, None, co, PLAIN)
        gemm(dgr, None, ci, mode)
        gemm(K.gather(n, h, w, 1, _src(co, False)), fwd, 0, 0)
        if dtype == F32:
            for g, c_in, c0, n_cols, m, s in ((fwd, ci, cins[0], co, PLAIN, 0), (dgr, co, co, ci, mode, split)):
                if K.query("selunet_conv3x3_x2_ok", h, w, c_in, c0, n_cols):
                    names.add(K.query("selunet_conv3x3_x2_kernel_name", ctypes.byref(g), n_cols, m, s).decode())
                if K.query("selunet_conv3x3_wino_ok", h, w, c_in, c0, n_cols):
                    names.add(K.query("selunet_conv3x3_wino_kernel_name", n_cols, m, s).decode())
    for (name, ci, co), d in zip(L.UNPOOLS, (8, 4, 2)):
        h, w = H // d, W // d
        up = K.gather(n, h, w, 1, _src(ci, True))
        dgr = K.gather(n, h, w, 4, _src(co, False))
        gemm(up, None, 4 * co, SCATTER)
        gemm(dgr, None, ci, PLAIN)
        gemm(K.gather(n, h, w, 1, _src(ci, True)), dgr, 0, 0)
    return names


def test_ledger_names_are_the_names_the_network_dispatches_to(lib):
    """The names of the ledger's rows equal the names collected over UNet_B's layer list at 256 x 256, 64 x 136 and
    40 x 56, in both dtypes, over HALO, HALO_PERSIST, WINO_WGRAD, X2D and X2P each at 0 and 1; the rows marked
    as out of the network's reach are exactly the other names the queries can return."""
    keys = ("HALO", "HALO_PERSIST", "WINO_WGRAD", "X2D", "X2P")
    seen = set()
    with _options(**DEFAULTS):
        for values in itertools.product((0, 1), repeat=len(keys)):
            with _options(**dict(zip(keys, values))):
                for H, W in ((256, 256), (64, 136), (40, 56)):
                    for dtype in (F32, BF16):
                        seen |= layer_names(2, H, W, dtype)
    in_net = {r[3] for r in LEDGER if r[5]}
    assert seen == in_net, (sorted(seen - in_net), sorted(in_net - seen))
    assert {r[3] for r in LEDGER} == ALL_NAMES
    assert not {r[3] for r in LEDGER if not r[5]} & seen


def test_every_option_only_variant_has_a_row():
    """The instantiations an option selects without changing the kernel name each have a row: the Winograd
    weight gradient's tile width and wave count, the fp32 halo weight gradient on split partials (an odd width,
    or WINO_WGRAD = 0), several pixel tiles per workgroup (WGRAD_WGS), the non-persistent halo kernel and the
    gather GEMM on halo-sized operands."""
    opts = [(r[0], r[1], r[3]) for r in LEDGER]
    for tw, nw in ((8, 12), (8, 8), (16, 8)):
        assert ({"WINO_WGRAD_TW": tw, "WINO_WGRAD_WAVES": nw}, F32, "conv3x3_wgrad_wino_f32<64>") in opts
    for bi in (128, 64):
        assert ({"WINO_WGRAD": 0}, F32, f"conv3x3_wgrad_halo_f32<{bi}>") in opts
        assert any(o == {} and n == f"conv3x3_wgrad_halo_f32<{bi}>" and r[2][3] % 2 == 1
                   for (o, _, n), r in zip(opts, LEDGER))
    for dt, tag in ((F32, "f32"), (BF16, "bf16")):
        for bn in (128, 64):
            assert ({"HALO_PERSIST": 0}, dt, f"conv3x3_halo<{tag},{bn}>") in opts
        assert ({"HALO": 0}, dt, f"gemm_gather<{tag}>") in opts
    assert any("WGRAD_WGS" in o for o, _, _ in opts)


# ------------------------------------------------------------------ option-induced rejections (before any launch)
def test_x2p_refuses_epilogues_it_cannot_route(lib):
    """SELUNET_OPT_X2P = 1: selunet_conv3x3_x2 with a SPLIT epilogue whose boundary is no multiple of 8, or with a
    scatter epilogue, returns EINVAL with a message; argument validation, so nothing is enqueued (the pointers
    here are never dereferenced)."""
    g = K.gather(2, 32, 32, 9, _src(128, True))
    with _options(**DEFAULTS), _options(X2P=1):
        assert kernel_name(F32, ("x2", 2, 32, 32, (128,), True, 128, PLAIN, 0)) == "conv3x3_x2p<f32,128>"
        for mode, split in ((SPLIT, 36), (SPLIT, 4), (SCATTER, 0)):
            ep = K.Epilogue(K.ptr(_FAKE), K.ptr(_FAKE), None, None, mode, split)
            rc = lib.selunet_conv3x3_x2(g, K.ptr(_FAKE), 128, ep, K.ptr(_FAKE), None, None)
            assert rc == 1, (mode, split)  # SELUNET_EINVAL
            assert lib.selunet_last_error(), (mode, split)
            with pytest.raises(K.SelunetError):
                K.call("selunet_conv3x3_x2", g, K.ptr(_FAKE), 128, ep, K.ptr(_FAKE), None, None)
