"""Whole-image prediction without a GPU: `predict.TilePlan`'s geometry and refusals, the argument rules of
`selunet_tile_gather` / `selunet_tile_stitch` (host-side, before any launch), and — on the CPU oracle — the
two facts the tiling rests on: the receptive field fits in HALO_MIN, and tiling with a halo
of 56 reproduces one forward of the whole reflect-padded image bit for bit, while a halo of 8 does not."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import unet_b_cpu as O
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import build as B
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR
from tests import _predict_ref as R

SIZES = [(1, 1), (100, 140), (400, 400), (401, 399)]


# ----------------------------------------------------------------------------- TilePlan
@pytest.mark.parametrize("tile,halo", [(160, 56), (512, 56), (64, 8), (128, 0)])
@pytest.mark.parametrize("H,W", SIZES)
def test_tile_plan_geometry(H, W, tile, halo):
    p = PR.TilePlan(H, W, tile, halo, allow_small_halo=True)
    core, grid, origins = R.grid_of(H, W, tile, halo)
    assert p.core == core == tile - 2 * halo and p.grid == grid and p.n == grid[0] * grid[1]
    assert p.origins.dtype == np.int32 and p.origins.flags["C_CONTIGUOUS"]
    assert np.array_equal(p.origins, origins)  # row-major (i core - halo, j core - halo)
    assert (p.origins % 8 == 0).all()
    assert (p.Hc, p.Wc) == (grid[0] * core, grid[1] * core)
    assert p.Hc >= H and p.Wc >= W and p.Hc - H < core and p.Wc - W < core and p.Wc % 8 == 0
    cover = np.zeros((p.Hc, p.Wc), np.int32)
    for y0, x0 in p.origins:
        assert 0 <= y0 + halo and y0 + tile - halo <= p.Hc and 0 <= x0 + halo and x0 + tile - halo <= p.Wc
        cover[y0 + halo:y0 + tile - halo, x0 + halo:x0 + tile - halo] += 1
    assert (cover == 1).all()  # the cores tile the canvas exactly once


def test_tile_plan_defaults_and_export():
    import selectivenet_for_semantic_segmentation_binary_amd as S
    assert S.TilePlan is PR.TilePlan and S.predict_image is PR.predict_image
    p = S.TilePlan(4096, 4096)
    assert (p.tile, p.halo, p.core, p.grid, p.n) == (512, 56, 400, (11, 11), 121)
    assert PR.HALO_MIN == 56


@pytest.mark.parametrize("kw,word", [
    (dict(halo=48), "HALO_MIN"), (dict(halo=8), "HALO_MIN"), (dict(halo=60), "multiple of 8"),
    (dict(halo=-8), "multiple of 8"), (dict(tile=164), "multiple of 8"), (dict(tile=112), "no core"),
    (dict(tile=104), "no core"), (dict(tile=520), "no fixture above"), (dict(H=0), "height and width"),
    (dict(W=65536), "height and width")])
def test_tile_plan_rejects_bad_arguments_with_a_message(kw, word):
    args = dict(H=100, W=140, tile=160, halo=56)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        PR.TilePlan(**args)


def test_tile_plan_small_halo_only_on_request():
    assert PR.TilePlan(100, 140, 64, 8, allow_small_halo=True).core == 48
    with pytest.raises(ValueError, match="multiple of 8"):  # the grid rule is not negotiable
        PR.TilePlan(100, 140, 64, 4, allow_small_halo=True)


# ----------------------------------------------------------------------------- C ABI argument rules
@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(K.lib_path()):
        B.build()
    return K.load()


A = 0x10000  # a 16-B aligned address that is never dereferenced: every call below is refused on the host


def gather_args(**kw):
    a = dict(img=A, H=37, W=53, origins=A, n=3, th=24, tw=32, mode=0, x=A, stream=None)
    a.update(kw)
    return [a[k] for k in ("img", "H", "W", "origins", "n", "th", "tw", "mode", "x", "stream")]


def stitch_args(**kw):
    a = dict(out=A, sel=A, origins=A, n=9, th=40, tw=48, halo=8, H=50, W=70, Hc=72, Wc=96, t_out=0.0, t_sel=0.0,
             logit_plane=A, sel_plane=A, mask=A, prob8=A, counts=A, stream=None)
    a.update(kw)
    return [a[k] for k in ("out", "sel", "origins", "n", "th", "tw", "halo", "H", "W", "Hc", "Wc", "t_out", "t_sel",
                           "logit_plane", "sel_plane", "mask", "prob8", "counts", "stream")]


GATHER_BAD = [dict(img=None), dict(origins=None), dict(x=None), dict(n=0), dict(n=-1), dict(H=0), dict(H=65536),
              dict(W=0), dict(W=65536), dict(th=0), dict(th=4), dict(th=20), dict(tw=4), dict(tw=36), dict(mode=-1),
              dict(mode=3), dict(x=A + 4), dict(x=A + 8)]
STITCH_BAD = [dict(out=None), dict(origins=None), dict(logit_plane=None), dict(mask=None), dict(counts=None),
              dict(sel=None), dict(sel_plane=None),  # sel and sel_plane: both or neither
              dict(n=0), dict(H=0), dict(H=65536), dict(W=0), dict(W=65536), dict(th=4), dict(th=44), dict(tw=4),
              dict(tw=52), dict(halo=4), dict(halo=12), dict(halo=-8), dict(halo=24), dict(halo=20, th=40, tw=64),
              dict(Hc=49), dict(Wc=64), dict(Wc=100), dict(out=A + 4), dict(sel=A + 8), dict(logit_plane=A + 4),
              dict(sel_plane=A + 8), dict(mask=A + 8), dict(prob8=A + 1)]


@pytest.mark.parametrize("bad", GATHER_BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_tile_gather_refuses_on_the_host(lib, bad):
    assert lib.selunet_tile_gather(*gather_args(**bad)) == 1
    assert b"tile_gather" in lib.selunet_last_error()
    with pytest.raises(K.SelunetError, match="tile_gather"):
        K.call("selunet_tile_gather", *gather_args(**bad))


@pytest.mark.parametrize("bad", STITCH_BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_tile_stitch_refuses_on_the_host(lib, bad):
    assert lib.selunet_tile_stitch(*stitch_args(**bad)) == 1
    assert b"tile_stitch" in lib.selunet_last_error()
    with pytest.raises(K.SelunetError, match="tile_stitch"):
        K.call("selunet_tile_stitch", *stitch_args(**bad))


def test_bindings_match_the_argument_counts(lib):
    assert len(K.SIGNATURES["selunet_tile_gather"][1]) == len(gather_args()) == 10
    assert len(K.SIGNATURES["selunet_tile_stitch"][1]) == len(stitch_args()) == 19
    assert K.SIGNATURES["selunet_tile_stitch"][1][11:13] == [ctypes.c_float, ctypes.c_float]


# ----------------------------------------------------------------------------- the oracle's facts
def test_reflect_index_is_numpy_reflect_padding():
    for n in (1, 2, 5, 9, 37):
        a = np.arange(n)
        for before, after in ((0, 0), (3, 4), (40, 60)):
            want = a if n == 1 and before + after == 0 else np.pad(a, (before, after), mode="reflect")
            assert np.array_equal(R.refl(np.arange(-before, n + after), n), want), (n, before, after)


def test_receptive_field_fits_in_halo_min():
    """The input pixels one output pixel of the eval-mode oracle depends on, by autograd, at all 8
    alignments of the pixel against the three poolings: 2+4+8+16+8+4+2 = 44 from the 3x3 convolutions plus
    at most 7 of pooling alignment."""
    params, buffers = O.make_state(0, "RGB", True)
    params = {k: v.detach() for k, v in params.items()}
    n = 192
    x = torch.randn(1, 3, n, n, generator=torch.Generator().manual_seed(0), requires_grad=True)
    out, sel, aux = O.forward(params, buffers, x, True, training=False)
    reach = 0
    for a in range(8):
        y0 = x0 = n // 2 + a
        (g,) = torch.autograd.grad(out[0, y0, x0] + sel[0, y0, x0] + aux[0, y0, x0], x, retain_graph=True)
        ys, xs = np.nonzero(g[0].abs().sum(0).numpy())
        r = max(y0 - ys.min(), ys.max() - y0, x0 - xs.min(), xs.max() - x0)
        assert 0 < ys.min() and ys.max() < n - 1 and 0 < xs.min() and xs.max() < n - 1  # the input was wide enough
        reach = max(reach, int(r))
    print(f"receptive field: reaches {reach} pixels to either side")
    assert 44 <= reach <= 51  # the count above
    assert reach <= PR.HALO_MIN and PR.HALO_MIN % 8 == 0


@pytest.fixture(scope="module")
def oracle_case():
    params, buffers = R.calibrated_state()
    forward = R.oracle_forward(params, buffers)
    image = R.sample_image(100, 140)
    out, sel = R.canvas_ref(forward, image, 56, 144, 144)  # one forward of the 256 x 256 reflect-padded canvas
    return {"forward": forward, "image": image, "out": out, "sel": sel}


def test_tiling_with_halo_56_is_exact_on_the_oracle(oracle_case):
    c = oracle_case
    p = PR.TilePlan(100, 140, 160, 56)
    assert (p.n, p.Hc, p.Wc) == (9, 144, 144)
    out, sel = R.predict_ref(c["forward"], c["image"], 160, 56)
    d = max(np.abs(out - c["out"]).max(), np.abs(sel - c["sel"]).max())
    print(f"halo 56, 9 tiles of 160: max |stitched - canvas forward| = {d}")
    assert np.array_equal(out, c["out"]) and np.array_equal(sel, c["sel"])
    assert np.ptp(c["out"]) > 0.1 and np.ptp(c["sel"]) > 0.1  # the heads spread: equality is not of constants


def test_tiling_with_halo_8_is_visibly_inexact_on_the_oracle(oracle_case):
    """The precondition of the GPU comparison (tests/test_gpu_predict.py, bound 1e-4 of max |logit|): a halo
    below the receptive field moves the logits by more than 10 times that bound."""
    c = oracle_case
    out, sel = R.predict_ref(c["forward"], c["image"], 64, 8)
    assert out.shape == c["out"].shape == (144, 144)
    e_out = np.abs(out - c["out"]).max() / np.abs(c["out"]).max()
    e_sel = np.abs(sel - c["sel"]).max() / np.abs(c["sel"]).max()
    print(f"halo 8, 9 tiles of 64: max rel error out {e_out:.2e}, sel {e_sel:.2e}")
    assert max(e_out, e_sel) > 10 * 1e-4
