"""The C-ABI boundary (include/selunet.h) without a GPU.

* every function the header declares is exported by libselunet.so and bound in `_lib.SIGNATURES`
  (and nothing is bound that the header does not declare);
* the ctypes mirrors of the header's structs have the C compiler's size and field offsets
  (a small C program built with gcc against the header prints them);
* the host-only entry points answer without touching a device (version, size queries,
  argument validation with a readable `selunet_last_error`);
* the product path refuses to run without the library (no CPU fallback).
"""
import ctypes
import os
import re
import subprocess

import pytest

from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import build as B

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "selunet.h")


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(selunet_[A-Za-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(K.lib_path()):
        B.build()
    return ctypes.CDLL(K.lib_path())


def test_header_declarations_are_exported_and_bound(lib):
    decl = _declared()
    assert len(decl) >= 30, decl
    missing = [f for f in decl if not hasattr(lib, f)]
    assert not missing, missing
    assert sorted(K.SIGNATURES) == decl


STRUCTS = {
    "selunet_source": (K.Source, ["data", "scale", "shift", "channels", "relu", "layout", "reserved"]),
    "selunet_gather": (K.Gather, ["n", "h", "w", "taps", "nsrc", "reserved", "src"]),
    "selunet_epilogue": (K.Epilogue, ["out0", "out1", "bias", "stats", "mode", "split", "colsum", "bnb"]),
    "selunet_bn_bwd_stats": (K.BnBwdStats, ["y", "scale", "shift", "mean", "invstd", "slab"]),
    "selunet_adam_tensor": (K.AdamTensor, ["param", "grad", "exp_avg", "exp_avg_sq", "numel", "chunk_begin"]),
}


def test_struct_layouts_match_the_c_compiler(tmp_path):
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){"]
    for s, (_, fields) in STRUCTS.items():
        src.append(f'printf("{s} size %zu\\n", sizeof({s}));')
        for f in fields:
            src.append(f'printf("{s} {f} %zu\\n", offsetof({s}, {f}));')
    src.append('printf("consts %d %d %d\\n", SELUNET_GEMM_BM, SELUNET_ADAM_CHUNK, SELUNET_EP_SCATTER2X);')
    src.append("return 0;}")
    c = tmp_path / "abi.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(line.split()[:2]): int(line.split()[2]) for line in out if line and not line.startswith("consts")}
    for s, (cls, fields) in STRUCTS.items():
        assert got[(s, "size")] == ctypes.sizeof(cls), s
        for f in fields:
            assert got[(s, f)] == getattr(cls, f).offset, (s, f)
    consts = [line for line in out if line.startswith("consts")][0].split()[1:]
    assert list(map(int, consts)) == [K.GEMM_BM, K.ADAM_CHUNK, K.EP_SCATTER2X]


def test_host_queries_need_no_device(lib):
    h = K.load()
    assert h.selunet_version() >= 1
    assert K.query("selunet_channel_slab_rows", 1 << 20) > 0
    assert K.query("selunet_loss_slab_rows", 1 << 20) > 0
    assert K.query("selunet_reduce_ws_bytes", 4) > 0
    assert K.query("selunet_wgrad_ld", 9 * 64) >= 9 * 64
    import torch
    fake = torch.empty(64, dtype=torch.bfloat16)  # never dereferenced: the query inspects shapes/alignment
    g = K.gather(2, 32, 32, 9, K.source(fake, 64))
    assert K.query("selunet_gemm_stats_rows", ctypes.byref(g), 64, K.BF16) in (2 * 2 * 2, 2 * 32 * 32 // K.GEMM_BM)
    g = K.gather(2, 8, 8, 1, K.source(fake, 64))  # 1x1 taps: generic kernel, one stats row per 128 pixels
    assert K.query("selunet_gemm_stats_rows", ctypes.byref(g), 64, K.BF16) == 1
    assert K.query("selunet_gemm_kernel_name", ctypes.byref(g), None, 64, K.EP_PLAIN, K.BF16) == b"gemm_gather<bf16>"
    # split-fp16 3x3 conv, 64 columns: the option SELUNET_OPT_X2D picks the kernel and its slab rows
    f32 = torch.empty(64, dtype=torch.float32)
    scale = torch.ones(64)
    fwd = K.gather(4, 64, 64, 9, K.source(f32, 64, scale, scale))  # BN+ReLU source: a forward
    dgr = K.gather(4, 64, 64, 9, K.source(f32, 64))
    name = lambda g: K.query("selunet_conv3x3_x2_kernel_name", ctypes.byref(g), 64, K.EP_PLAIN, 0)  # noqa: E731
    rows = lambda g: K.query("selunet_conv3x3_x2_stats_rows", ctypes.byref(g), 64)  # noqa: E731
    prev = K.set_option("X2D", -1)
    try:
        assert name(fwd) == b"conv3x3_x2d<f32,64>" and rows(fwd) == 4 * 4 * 4  # one row per 16x16 tile
        assert name(dgr) == b"conv3x3_x2<f32,64>"
        K.set_option("X2D", 0)
        assert name(fwd) == b"conv3x3_x2<f32,64>"
        K.set_option("X2D", 1)
        assert name(dgr) == b"conv3x3_x2d<f32,64>"
    finally:
        K.set_option("X2D", prev)


def _cdiv(a, b):
    return -(-a // b)


def _splits(total, groups, target=256):
    """The pixel-tile split plan of the 3x3 weight gradients, restated: about `target` workgroups over
    (co tile, ci chunk, split), every split taking the same `per` pixel tiles."""
    want = max(1, _cdiv(max(1, target), groups))
    per = _cdiv(total, min(total, want))
    return _cdiv(total, per)


class _options:
    """Set options by name for a block (value -1: the default) and put the previous values back."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.prev = [(k, K.set_option(k, v)) for k, v in self.kv.items()]

    def __exit__(self, *exc):
        for k, v in reversed(self.prev):
            K.set_option(k, v)


# (n, h, w, co, Q source channels); the fourth has fewer pixel tiles than the plan wants splits
WGRAD_SHAPES = [(16, 256, 256, 64, (64,)), (16, 128, 128, 128, (128,)), (2, 16, 24, 256, (128,)),
                (1, 8, 16, 64, (64,)), (128, 32, 32, 512, (512,)), (2, 16, 24, 128, (64, 64))]


def test_wgrad_split_plans_without_a_device(lib):
    """The host-side planning of the 3x3 weight gradients, pinned against a restatement: the workspace
    queries give splits * ni * row * 4 bytes with the split plan above, per path (its column tile, pixel
    tile, row length and workgroup-target option)."""
    import torch
    K.load()
    fake = torch.empty(64, dtype=torch.float32)  # never dereferenced

    def operands(n, h, w, co, cis):
        gp = K.gather(n, h, w, 1, K.source(fake, co))
        gq = K.gather(n, h, w, 9, *[K.source(fake, c) for c in cis])
        return ctypes.byref(gp), ctypes.byref(gq), (gp, gq)

    def tiles(n, h, w, th, tw):
        return n * _cdiv(h, th) * _cdiv(w, tw)

    def bi(co):
        return 128 if co % 128 == 0 else 64

    base = dict(HALO=-1, WGRAD_WGS=-1, X2_WGRAD_WGS=-1, WINO_WGRAD=-1, WINO_WGRAD_TW=-1)
    x2_splits = []
    with _options(**base):
        for n, h, w, co, cis in WGRAD_SHAPES:
            ci = sum(cis)
            p, q, _keep = operands(n, h, w, co, cis)
            ld = K.query("selunet_wgrad_ld", 9 * ci)
            groups = (co // bi(co)) * (ci // 64)
            # split-fp16: 128- or 64-column tiles of 8x8 pixels, partial rows of ld floats
            s = _splits(tiles(n, h, w, 8, 8), groups)
            x2_splits.append(s)
            assert K.query("selunet_conv3x3_wgrad_x2_ws_bytes", p, q) == s * co * ld * 4, (n, h, w, co, cis)
            # fp32 Winograd: 64-column tiles of 8x16 pixels, partial rows of the 12 planes
            s = _splits(tiles(n, h, w, 8, 16), (co // 64) * (ci // 64))
            assert K.query("selunet_gemm_wgrad_ws_bytes", p, q, K.F32) == s * co * 12 * ci * 4, (n, h, w, co, cis)
            # fp32 halo: 8x8 pixels; bf16 halo: 8x16 pixels
            with _options(WINO_WGRAD=0):
                s = _splits(tiles(n, h, w, 8, 8), groups)
                assert K.query("selunet_gemm_wgrad_ws_bytes", p, q, K.F32) == s * co * ld * 4, (n, h, w, co, cis)
            s = _splits(tiles(n, h, w, 8, 16), groups)
            assert K.query("selunet_gemm_wgrad_ws_bytes", p, q, K.BF16) == s * co * ld * 4, (n, h, w, co, cis)
        assert x2_splits[:5] == [256, 128, 12, 2, 8]
        # each path follows its own workgroup-target option
        n, h, w, co, cis = WGRAD_SHAPES[1]
        p, q, _keep = operands(n, h, w, co, cis)
        ld = K.query("selunet_wgrad_ld", 9 * 128)
        want_x2 = {t: _splits(tiles(n, h, w, 8, 8), 2, t) * co * ld * 4 for t in (64, 256)}
        want_bf = {t: _splits(tiles(n, h, w, 8, 16), 2, t) * co * ld * 4 for t in (64, 256)}
        want_wi = {t: _splits(tiles(n, h, w, 8, 16), 4, t) * co * 12 * 128 * 4 for t in (64, 256)}
        assert want_x2[64] != want_x2[256] and want_bf[64] != want_bf[256]
        with _options(X2_WGRAD_WGS=64):
            assert K.query("selunet_conv3x3_wgrad_x2_ws_bytes", p, q) == want_x2[64]
            assert K.query("selunet_gemm_wgrad_ws_bytes", p, q, K.BF16) == want_bf[256]
        with _options(WGRAD_WGS=64):
            assert K.query("selunet_conv3x3_wgrad_x2_ws_bytes", p, q) == want_x2[256]
            assert K.query("selunet_gemm_wgrad_ws_bytes", p, q, K.BF16) == want_bf[64]
            assert K.query("selunet_gemm_wgrad_ws_bytes", p, q, K.F32) == want_wi[64]
        assert K.query("selunet_conv3x3_wgrad_x2_ws_bytes", p, q) == want_x2[256]
        assert K.query("selunet_gemm_wgrad_ws_bytes", p, q, K.BF16) == want_bf[256]


def test_x2_forward_geometry_without_a_device(lib):
    """The split-fp16 3x3 forward on 128-column tiles: kernel name, the tile-width predicate under a SPLIT
    epilogue (beside the Winograd kernel's), and the statistics rows of either tile schedule."""
    import torch
    fake = torch.empty(64, dtype=torch.float32)  # never dereferenced
    name = lambda g, nc, mode=K.EP_PLAIN, split=0: K.query(  # noqa: E731
        "selunet_conv3x3_x2_kernel_name", ctypes.byref(g), nc, mode, split)
    rows = lambda g, nc: K.query("selunet_conv3x3_x2_stats_rows", ctypes.byref(g), nc)  # noqa: E731
    wino = lambda nc, mode, split: K.query("selunet_conv3x3_wino_kernel_name", nc, mode, split)  # noqa: E731
    big = K.gather(16, 128, 128, 9, K.source(fake, 128))   # 1024 pixel tiles of 16x16
    odd = K.gather(2, 20, 24, 9, K.source(fake, 128))      # 8 pixel tiles
    wgs = K.query("selunet_set_halo_workgroups", 256)
    try:
        with _options(HALO=-1, HALO_PERSIST=-1, X2D=-1, TILE_QUEUE=0):
            for nc in (128, 256, 512):
                assert name(big, nc) == b"conv3x3_x2<f32,128>"
                assert rows(big, nc) == min(1024, 256 // (nc // 128))
                assert rows(odd, nc) == min(8, 256 // (nc // 128))
            assert name(big, 192) == b"conv3x3_x2<f32,64>" and rows(big, 192) == 256
            # a SPLIT epilogue keeps 128 columns at any split the LDS-staged epilogue can route (a multiple
            # of 8); the Winograd kernel's register epilogue needs the split on a tile boundary
            assert name(big, 128, K.EP_SPLIT, 64) == b"conv3x3_x2<f32,128>"
            assert name(big, 128, K.EP_SPLIT, 68) == b"conv3x3_x2<f32,64>"
            assert wino(256, K.EP_SPLIT, 128) == b"conv3x3_wino<f32,128>"
            assert wino(128, K.EP_SPLIT, 64) == b"conv3x3_wino<f32,64>"
            assert wino(128, K.EP_PLAIN, 0) == b"conv3x3_wino<f32,128>"
            assert wino(192, K.EP_PLAIN, 0) == b"conv3x3_wino<f32,64>"
            # the ticket-counter schedule flushes statistics per pixel tile; its counters live on a device,
            # so without one the option is refused and only the static half above is checked
            if K.set_option("TILE_QUEUE", 1) >= 0:
                assert name(big, 256) == b"conv3x3_x2<f32,128>"
                assert rows(big, 256) == 1024 and rows(odd, 256) == 8
    finally:
        K.query("selunet_set_halo_workgroups", wgs)


def test_invalid_arguments_fail_with_a_message(lib):
    h = K.load()
    # unsupported channel count for the BN reduction: rejected on the host before any launch
    rc = h.selunet_channel_sum(None, 10, 3, None, K.F32, None)
    assert rc == 1
    assert h.selunet_last_error()
    with pytest.raises(RuntimeError):
        K.call("selunet_channel_sum", None, 10, 3, None, K.F32, None)


def test_product_path_has_no_cpu_fallback():
    import torch

    import selectivenet_for_semantic_segmentation_binary_amd as S
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    net = S.UNet_B("RGB", selective=True)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError):
        S.calc_selective_risk_image_b(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4))


def test_build_id_carries_the_sources_and_the_arch(lib, tmp_path):
    """the library's build id is '<source fingerprint> <arch>'; the fingerprint leaves the
    target arch out (a library built for another SELUNET_ARCH is reported as such), and the .sha stamp
    next to the library is what load(auto_build=True) compares before mapping it (stale -> rebuild)."""
    lib.selunet_build_id.restype = ctypes.c_char_p
    fp, arch = B.parse_build_id(lib.selunet_build_id().decode())
    assert fp == B.source_fingerprint() and arch == B.ARCH
    assert B.lib_stamp_fingerprint(K.lib_path()) == fp
    stamp = tmp_path / "x.so.sha"
    stamp.write_text("0123abcd gfx942")
    assert B.lib_stamp_fingerprint(str(tmp_path / "x.so")) == "0123abcd"
    assert B.lib_stamp_fingerprint(str(tmp_path / "missing.so")) is None
    assert not any("offload-arch" in f for f in B.BASE_FLAGS)
