"""The grid-stride I/O, metrics and prediction kernels where their loops wrap: every launch that sizes its grid with
io_grid (csrc/common.h) under SELUNET_OPT_IO_GRID = 3 and = 1, at sizes where three workgroups (768 threads) make
at least three passes and a ragged last one (tests/test_io_regimes_host.py holds the arithmetic). At the default
grid these sizes are one pass; whole-slide prediction wraps every one of these loops many times.

For each entry point: the outputs under 3 and 1 are torch.equal to the default grid's, atomically accumulated
counts included; the default grid's equal the module's existing reference by its existing rule; outputs are
NaN- or sentinel-filled first, so an element left unwritten or written outside its range shows; the accumulating
calls are also run twice."""
import numpy as np
import pytest
import torch

from oracle import data_cpu as OD
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from selectivenet_for_semantic_segmentation_binary_amd import data as D
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR
from tests import _boundary_ref as BR
from tests import _patch_ref as PRF
from tests import _predict_ref as R
from tests import _regions_ref as RR
from tests import _tissue_ref as TS
from tests import _tta_ref as TR
from tests.test_gpu_boundary import blobs
from tests.test_gpu_predict_tta import EDGE, GATHER_ORIGINS, same
from tests.test_gpu_regions_tiles import label_filled
from tests.test_gpu_sweep import edge_case
from tests.test_gpu_tissue import edge_image, pitched

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
T_OUT = F32(MT.logit_threshold("eval", 0.5))
T_SEL = F32(MT.logit_threshold("eval", 0.7))
GRIDS = (-1, 3, 1)
TPB = 256  # IO_TPB, PRED_TPB, BND_TPB
# work items (threads' loop trips) of each launch at the sizes below, by the kernels' own formulas
ITEMS = {
    "prep_batch": 5 * 24 * (80 // 4),               # n h (w / 4)
    "seg_metrics": (16 * 603 - 1) // 4 + 1,         # p / 4 + 1
    "seg_metrics_rows": 16 * 603 // 4,              # hw / 4 per image
    "tile_gather": 7 * 24 * (56 // 4),              # n th (tw / 4)
    "tile_gather_flip": 7 * 40 * (40 // 4),
    "tile_stitch": 25 * 24 * (32 // 8),             # n core rows (core columns / 8)
    "tta_accumulate": 35 * 24 * (24 // 8 + 1),      # n core rows (core columns / 8 + 1)
    "tissue_plane": 70 * 35,                        # h (pitch / 4)
    "tissue_class_counts": 70 * 35,                 # h cdiv(w, 4)
    "regions_flatten": 70 * 35,                     # h (label pitch / 4)
    "regions_apply": 70 * 35,
    "boundary_bands": 2 * 97 * 101 // 4 + 1,        # p / 4 + 1
    "boundary_rows": 97 * 101 // 4,                 # hw / 4 per image
}


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def wraps(items):
    """The regime every size here is chosen for: three workgroups make >= 3 full passes and a ragged last one."""
    assert items > 3 * 3 * TPB and items % (3 * TPB) and items % TPB, items


for _items in ITEMS.values():
    wraps(_items)


def under_grids(run):
    """run() -> {name: device tensor} at IO_GRID = -1, 3 and 1 (the previous value restored); the capped runs must
    equal the default one bit for bit. Returns the default run's tensors."""
    prev = K.set_option("IO_GRID", -1)
    try:
        res = []
        for g in GRIDS:
            K.set_option("IO_GRID", g)
            assert K.set_option("IO_GRID", g) == g  # the option reads back
            res.append(run())
            torch.cuda.synchronize()
    finally:
        K.set_option("IO_GRID", prev)
    for g, r in zip(GRIDS[1:], res[1:]):
        for k, v in res[0].items():
            eq = torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v,
                             r[k].view(torch.int32) if v.dtype == torch.float32 else r[k])
            assert eq, f"IO_GRID = {g}: {k} differs from the default grid's"
    return {k: v.cpu().numpy() for k, v in res[0].items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ----------------------------------------------------------------------------- train_io.hip
@pytest.mark.parametrize("input_type", ["RGB", "GH", "H_RGB"])
def test_prep_batch(input_type):
    """selunet_prep_batch (RGB, GH) and selunet_prep_batch_mode (H_RGB) with every flip, against oracle/data_cpu.py:
    RGB and the labels bit for bit, GH within 1e-6 / 1e-5, H_RGB within 1e-5 (tests/test_gpu_data.py's rules)."""
    n, h, w = 5, 24, 80
    assert n * h * (w // 4) == ITEMS["prep_batch"]
    rng = np.random.Generator(np.random.PCG64(80))
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    lab = rng.choice(np.array([0, 1, 127, 254, 255], np.uint8), (n, h, w))
    flips = np.array([0, 1, 2, 3, 1], np.uint8)
    cin = 2 if input_type == "GH" else 3
    di, dl, df = dev(img), dev(lab), dev(flips)

    def run():
        x = torch.full((n, cin, h, w), float("nan"), device=DEV)
        t = torch.full((n, h, w), float("nan"), device=DEV)
        if input_type == "H_RGB":
            K.call("selunet_prep_batch_mode", K.ptr(di), K.ptr(dl), K.ptr(df), n, h, w, 2, K.ptr(x), K.ptr(t),
                   K.stream_ptr())
        else:
            K.call("selunet_prep_batch", K.ptr(di), K.ptr(dl), K.ptr(df), n, h, w, cin, K.ptr(x), K.ptr(t),
                   K.stream_ptr())
        return {"x": x, "t": t}

    got = under_grids(run)
    assert not np.isnan(got["x"]).any() and not np.isnan(got["t"]).any()
    conv = {"RGB": lambda a: a, "GH": OD.rgb2gh, "H_RGB": OD.h_rgb}[input_type]
    want = [OD.transform(conv((img[i] / 255.0).astype(F32)), (lab[i] / 255.0).astype(np.uint8), int(flips[i]))
            for i in range(n)]
    xe, te = np.stack([a for a, _ in want]), np.stack([b for _, b in want])
    assert np.array_equal(got["t"], te)
    if input_type == "RGB":
        assert np.array_equal(bits(got["x"]), bits(xe))
    elif input_type == "GH":
        assert np.abs(got["x"][:, 0] - xe[:, 0]).max() <= 1e-6 and np.abs(got["x"][:, 1] - xe[:, 1]).max() <= 1e-5
    else:
        assert np.abs(got["x"] - xe).max() <= 1e-5
    # flips NULL: every image as image 0 (flip 0) is above. (data.prep_batch allocates its outputs itself, so these are
    # not NaN-filled: they are held only against the un-flipped slices of the filled run above.)
    plain = under_grids(lambda: dict(zip(("x", "t"), D.prep_batch(di, dl, None, input_type))))
    unflip = lambda a, f: a[..., ::-1 if f & 2 else 1, ::-1 if f & 1 else 1]  # noqa: E731
    for i in range(n):
        assert np.array_equal(bits(unflip(got["x"][i], flips[i])), bits(plain["x"][i])), i
        assert np.array_equal(unflip(got["t"][i], flips[i]), plain["t"][i]), i


def metrics_case(parts, seed):
    """`parts` edge_case()s of 603 pixels each, concatenated: thresholds' neighbours, +-0, +-inf, NaN, labels >= 2."""
    cs = [edge_case(np.array([T_SEL], F32), seed + i) for i in range(parts)]
    return tuple(np.concatenate([c[j] for c in cs]) for j in range(3))


@pytest.mark.parametrize("selective", [True, False])
def test_seg_metrics(selective):
    """p % 4 == 3 (the scalar tail under a capped grid), with and without the selection head; two calls add."""
    out, sel, tgt = (a[:-1] for a in metrics_case(16, 100))
    p = out.size
    assert p % 4 == 3
    assert p // 4 + 1 == ITEMS["seg_metrics"]
    o, s, t = dev(out), dev(sel) if selective else None, dev(tgt)

    def run():
        counts = torch.zeros(2, 6, dtype=torch.int64, device=DEV)
        for calls in (1, 2):
            for _ in range(calls):
                K.call("selunet_seg_metrics", K.ptr(o), K.ptr(s), K.ptr(t), p, float(T_OUT), float(T_SEL),
                       K.ptr(counts[calls - 1]), K.stream_ptr())
        return {"counts": counts}

    got = under_grids(run)["counts"]
    want = np.array(PRF.numpy_counts(out, sel if selective else None, tgt, T_OUT, T_SEL), np.int64)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], 2 * want)
    assert want[:4].min() > 0 and (not selective or 0 < want[4] < p)


@pytest.mark.parametrize("selective", [True, False])
def test_every_entry_point_applies_one_pixel_rule(selective):
    """Two images of 36 x 36 = 1296 pixels (a multiple of 4, two passes of patch_auc's 1024 threads, six of one
    256-thread workgroup at IO_GRID = 1). Image 0 opens with every combination of an edge value of `out` (the two
    thresholds, their fp32 neighbours, +-0, +-inf, NaN, +-40), an edge value of `sel` and a label of 0, 1, 2, 3, 255;
    the rest is metrics_case's. The six selunet_seg_metrics counts equal the rule restated here in numpy, and every
    other entry point's totals of the same pixels equal them."""
    n, h, w = 2, 36, 36
    hw, p = h * w, n * h * w
    out, sel, tgt = (a[:p].copy() for a in metrics_case(5, 300))
    edge = out[:13].copy()  # edge_case's 13 values
    assert np.isnan(edge).sum() == 1 and {float(T_OUT), float(T_SEL), np.inf, -np.inf} <= set(edge.tolist())
    labels = np.array([0, 1, 2, 3, 255], F32)
    combos = edge.size ** 2 * labels.size
    assert combos <= hw
    out[:combos] = np.repeat(edge, edge.size * labels.size)
    sel[:combos] = np.tile(np.repeat(edge, labels.size), edge.size)
    tgt[:combos] = np.tile(labels, edge.size ** 2)

    # the rule: label = uint8(target); selected iff no selection plane or sel >= t_sel; pred = out >= t_out
    lab = tgt.astype(np.uint8)
    with np.errstate(invalid="ignore"):
        selected = sel >= T_SEL if selective else np.ones(p, bool)
        pred = out >= T_OUT
    cm = [int((selected & (lab == l) & (pred == q)).sum()) for l in (0, 1) for q in (False, True)]
    want = np.array(cm + [int(selected.sum()), p], np.int64)
    nan_pos = int((selected & (lab == 1) & np.isnan(out)).sum())
    assert min(cm) > 0 and nan_pos > 0 and want[4] - sum(cm) > 0 and (not selective or want[4] < p)

    shape = lambda a: a.reshape(n, h, w)  # noqa: E731
    o, s_all, t = dev(shape(out)), dev(shape(sel)), dev(shape(tgt))
    s = s_all if selective else None
    d2t, d2p = MT.boundary_distance_sq(t, 0.5), MT.boundary_distance_sq(o, float(T_OUT))
    r2 = (K.c_int32 * 2)(4, 100)
    thr = dev(np.array([T_SEL], F32))
    edges = dev(np.array([T_OUT], F32))
    args = (float(T_OUT), float(T_SEL))

    def run():
        z = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device=DEV)  # noqa: E731
        r = {"counts": z(6), "rows": z(n, 6), "sweep": z(2, 5), "bands": z(4, 6), "brows": z(n, 6), "auc": z(n, 4),
             "calib": z(2, 5), "misc": z(2)}
        st = K.stream_ptr()
        K.call("selunet_seg_metrics", K.ptr(o), K.ptr(s), K.ptr(t), p, *args, K.ptr(r["counts"]), st)
        K.call("selunet_seg_metrics_rows", K.ptr(o), K.ptr(s), K.ptr(t), n, hw, *args, K.ptr(r["rows"]), st)
        K.call("selunet_seg_metrics_sweep", K.ptr(o), K.ptr(s_all), K.ptr(t), p, float(T_OUT), K.ptr(thr), 1,
               K.ptr(r["sweep"]), st)
        K.call("selunet_boundary_bands", K.ptr(o), K.ptr(s), K.ptr(t), K.ptr(d2t), n, hw, *args, r2, 2,
               K.ptr(r["bands"]), st)
        K.call("selunet_boundary_rows", K.ptr(o), K.ptr(s), K.ptr(t), K.ptr(d2t), K.ptr(d2p), n, hw, *args, 4,
               K.ptr(r["brows"]), st)
        K.call("selunet_patch_auc", K.ptr(o), K.ptr(s), K.ptr(t), n, hw, float(T_SEL), K.ptr(r["auc"]), st)
        K.call("selunet_calibration_bins", K.ptr(o), None, K.ptr(s), K.ptr(t), p, 0, *args, K.ptr(edges), 1, 1.0,
               K.ptr(r["calib"]), None, K.ptr(r["misc"]), st)
        return r

    got = under_grids(run)
    assert np.array_equal(got["counts"], want)
    assert np.array_equal(got["rows"].sum(0), want)
    assert np.array_equal(got["bands"].sum(0), want)
    # the sweep has no "no selection plane": its bin 1 is what t_sel selects, both bins together are every pixel
    sweep = got["sweep"][1] if selective else got["sweep"].sum(0)
    assert np.array_equal(sweep, want[:5]) and got["sweep"][:, 4].sum() == p
    assert (got["brows"][:, 4].sum(), got["brows"][:, 5].sum()) == (want[1], want[2])  # fp = cm01, fn = cm10
    assert got["auc"][:, 1:].sum() == want[:4].sum()  # n_pos + n_neg + n_nan: the counted pixels
    non_events, events = got["calib"][:, 0].sum(), got["calib"][:, 1].sum()
    nan_scores, other_labels = got["misc"]
    assert events + nan_pos == want[2] + want[3]
    assert non_events + events + nan_scores == want[:4].sum()
    assert want[4] == want[:4].sum() + other_labels
    # one edge at t_out: bin 1 holds the pixels predicted 1 (a NaN score predicts 0 and is in no bin)
    assert (got["calib"][1, 0], got["calib"][1, 1]) == (want[1], want[3])


@pytest.mark.parametrize("selective", [True, False])
def test_seg_metrics_rows(selective):
    """Three images of 9648 pixels: gx = 3 by the launcher's own rule, so IO_GRID = 1 wraps what it does not."""
    n = 3
    cases = [metrics_case(16, 200 + 16 * i) for i in range(n)]
    out, sel, tgt = (np.stack([c[j] for c in cases]) for j in range(3))
    hw = out.shape[1]
    assert hw % 4 == 0
    assert hw // 4 == ITEMS["seg_metrics_rows"]
    o, s, t = dev(out), dev(sel) if selective else None, dev(tgt)

    def run():
        rows = torch.zeros(2, n, 6, dtype=torch.int64, device=DEV)
        for calls in (1, 2):
            for _ in range(calls):
                K.call("selunet_seg_metrics_rows", K.ptr(o), K.ptr(s), K.ptr(t), n, hw, float(T_OUT), float(T_SEL),
                       K.ptr(rows[calls - 1]), K.stream_ptr())
        return {"rows": rows}

    got = under_grids(run)["rows"]
    want = np.array([PRF.numpy_counts(out[i], sel[i] if selective else None, tgt[i], T_OUT, T_SEL) for i in range(n)],
                    np.int64)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], 2 * want)


# ----------------------------------------------------------------------------- predict_io.hip, predict_tta.hip
def gather_image():
    return np.random.Generator(np.random.PCG64(3753)).integers(0, 256, (37, 53, 3), dtype=np.uint8)


@pytest.mark.parametrize("input_type", ["RGB", "GH", "H_RGB"])
def test_tile_gather(input_type):
    """Seven 24 x 56 tiles of a 37 x 53 image, origins that fold several times: equal to prep_batch of the numpy
    crops, bit for bit (tests/test_gpu_predict.py's rule)."""
    image, th, tw = gather_image(), 24, 56
    n = len(GATHER_ORIGINS)
    assert n * th * (tw // 4) == ITEMS["tile_gather"]
    crops = R.crops(image, GATHER_ORIGINS, th, tw)
    want, _ = D.prep_batch(dev(crops), dev(np.zeros(crops.shape[:3], np.uint8)), None, input_type)
    di, do = dev(image), dev(GATHER_ORIGINS)

    def run():
        x = torch.full(tuple(want.shape), float("nan"), device=DEV)
        return {"x": PR.tile_gather(di, do, th, tw, input_type, out=x)}

    got = under_grids(run)["x"]
    assert not np.isnan(got).any() and np.array_equal(bits(got), bits(want.cpu().numpy()))


@pytest.mark.parametrize("input_type", ["RGB", "GH", "H_RGB"])
def test_tile_gather_flip(input_type):
    """Seven 40 x 40 tiles under the four flips: equal to the gather of the flipped image."""
    image, th = gather_image(), 40
    n = len(GATHER_ORIGINS)
    assert n * th * (th // 4) == ITEMS["tile_gather_flip"]
    di, do = dev(image), dev(GATHER_ORIGINS)
    want = [PR.tile_gather(dev(TR.T(k, image)), do, th, th, input_type).cpu().numpy() for k in range(4)]
    assert len({w.tobytes() for w in want}) == 4

    def run():
        res = {}
        for k in range(4):
            x = torch.full(want[0].shape, float("nan"), device=DEV)
            res[f"flip{k}"] = PR.tile_gather_flip(di, do, th, th, input_type, k, out=x)
        return res

    got = under_grids(run)
    for k in range(4):
        assert np.array_equal(bits(got[f"flip{k}"]), bits(want[k])), k


H_S, W_S, TILE_S, HALO_S = 110, 150, (40, 48), 8


def stitch_tiles(seed, n, th, tw, halo):
    """Scores ~ N(0, 3) with, along the first rows of every core, each threshold, its two fp32 neighbours, +-0,
    +-inf, NaN and saturated values in both heads (tests/test_gpu_predict.py's stitch_case, for any grid)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = rng.normal(0, 3, (n, th, tw)).astype(F32)
    sel = rng.normal(0, 3, (n, th, tw)).astype(F32)
    k = min(len(EDGE), tw - 2 * halo)
    for t in range(n):
        e = np.roll(EDGE, -t)[:k]
        out[t, halo, halo:halo + k] = e
        sel[t, halo + 1, halo:halo + k] = e
        out[t, halo + 2, halo:halo + k] = e
        sel[t, halo + 2, halo:halo + k] = e[::-1]
    return out, sel


@pytest.mark.parametrize("selective", [True, False])
def test_tile_stitch(selective):
    """25 tiles of 40 x 48 (cores of 24 x 32, canvas 120 x 160) over a 110 x 150 image: the four planes and the counts
    equal numpy (prob8 through the logits' bits: it is a function of them alone); two calls count twice."""
    th, tw = TILE_S
    ch, cw = th - 2 * HALO_S, tw - 2 * HALO_S
    origins = np.array([(i * ch - HALO_S, j * cw - HALO_S) for i in range(5) for j in range(5)], np.int32)
    n, Hc, Wc = len(origins), 5 * ch, 5 * cw
    assert n * ch * (cw // 8) == ITEMS["tile_stitch"]
    out, sel = stitch_tiles(21, n, th, tw, HALO_S)
    lp, sp = R.stitch(out, origins, HALO_S, Hc, Wc), R.stitch(sel, origins, HALO_S, Hc, Wc)
    mask = TR.mask_of(lp, sp if selective else None, T_OUT, T_SEL)
    want_counts = TR.counts_of(mask[:H_S, :W_S])
    assert min(want_counts[:2]) > 100
    o, s, do = dev(out), dev(sel) if selective else None, dev(origins)

    def run():
        logit = torch.full((Hc, Wc), -777.0, device=DEV)
        selp = torch.full((Hc, Wc), -777.0, device=DEV) if selective else None
        m = torch.full((Hc, Wc), 77, dtype=torch.uint8, device=DEV)
        prob8 = torch.full((Hc, Wc), 77, dtype=torch.uint8, device=DEV)
        counts = torch.zeros(4, dtype=torch.int64, device=DEV)
        PR.tile_stitch(o, s, origins, do, HALO_S, H_S, W_S, float(T_OUT), float(T_SEL), logit, selp, m, prob8, counts)
        once = counts.clone()
        PR.tile_stitch(o, s, origins, do, HALO_S, H_S, W_S, float(T_OUT), float(T_SEL), logit, selp, m, prob8, counts)
        res = {"logit": logit, "mask": m, "prob8": prob8, "once": once, "twice": counts}
        if selective:
            res["selection"] = selp
        return res

    got = under_grids(run)
    assert np.array_equal(bits(got["logit"]), bits(lp))  # the cores tile the canvas: no -777 is left
    if selective:
        assert np.array_equal(bits(got["selection"]), bits(sp))
    assert np.array_equal(got["mask"], mask)
    x = lp.astype(np.float64)
    nan = np.isnan(x)
    with np.errstate(over="ignore"):
        level = np.floor(255.0 / (1.0 + np.exp(-x[~nan])) + 0.5).astype(np.int64)
    assert np.abs(got["prob8"][~nan].astype(np.int64) - level).max() <= 1 and (got["prob8"][nan] == 0).all()
    assert got["once"].tolist() == want_counts and got["twice"].tolist() == [2 * v for v in want_counts]


H_A, W_A, TILE_A, HALO_A = 117, 149, 40, 8


@pytest.mark.parametrize("selective", [True, False])
def test_tta_accumulate(selective):
    """Members 0 (stored), 3 (both flips, added) and 3 again, 35 tiles of 40 x 40 each over a 117 x 149 image
    (w % 8 = 5: flipped cores start inside a group): sums and votes equal numpy; outside the image as it was."""
    core, grid, origins = R.grid_of(H_A, W_A, TILE_A, HALO_A)
    origins = origins.astype(np.int32)
    n, Hc, Wc = len(origins), grid[0] * core, grid[1] * core
    assert grid == (5, 7)
    assert n * core * (core // 8 + 1) == ITEMS["tta_accumulate"]
    rows, ws = H_A + 3, 152
    tiles = [stitch_tiles(31 + f, n, TILE_A, TILE_A, HALO_A) for f in (0, 3)]
    planes = [tuple(np.ascontiguousarray(TR.T_inv(f, R.stitch(v, origins, HALO_A, Hc, Wc)[:H_A, :W_A])) for v in tl)
              for f, tl in zip((0, 3), tiles)]
    with np.errstate(invalid="ignore", over="ignore"):
        sums = [(planes[0][i] + planes[1][i], (planes[0][i] + planes[1][i]) + planes[1][i]) for i in range(2)]
    votes = [[TR.votes_of([p[i] for p in planes[:1] + planes[1:] * k], t) for k in (1, 2)]
             for i, t in ((0, T_OUT), (1, T_SEL))]
    dt = [(dev(a), dev(b) if selective else None) for a, b in tiles]
    do = dev(origins)

    def run():
        s_out = torch.full((rows, ws), -777.0, device=DEV)
        s_sel = torch.full((rows, ws), -777.0, device=DEV) if selective else None
        v_out = torch.full((rows, ws), 77, dtype=torch.uint8, device=DEV)
        v_sel = torch.full((rows, ws), 77, dtype=torch.uint8, device=DEV) if selective else None
        res = {}
        for step, (m, f) in enumerate(((0, 0), (1, 3), (1, 3))):
            PR.tta_accumulate(dt[m][0], dt[m][1], origins, do, HALO_A, f, step == 0, H_A, W_A, Hc, Wc, float(T_OUT),
                              float(T_SEL), s_out, s_sel, v_out, v_sel)
            if step:
                res[f"sum_out{step}"], res[f"votes{step}"] = s_out.clone(), v_out.clone()
                if selective:
                    res[f"sum_sel{step}"], res[f"sel_votes{step}"] = s_sel.clone(), v_sel.clone()
        return res

    got = under_grids(run)
    for step in (1, 2):
        for i, (sk, vk) in enumerate((("sum_out", "votes"), ("sum_sel", "sel_votes"))[:2 if selective else 1]):
            g, v = got[f"{sk}{step}"], got[f"{vk}{step}"]
            assert same(g[:H_A, :W_A], sums[i][step - 1]), (sk, step)
            assert np.array_equal(v[:H_A, :W_A], votes[i][step - 1]), (vk, step)
            g, v = g.copy(), v.copy()
            g[:H_A, :W_A], v[:H_A, :W_A] = -777.0, 77
            assert (g == -777.0).all() and (v == 77).all(), (sk, step)  # words outside the image: as they were


# ----------------------------------------------------------------------------- predict_tissue.hip, predict_regions.hip
H_T, W_T = 70, 139  # W % 4 = 3: the last group of a row is ragged, rows start at every byte alignment


def test_tissue_plane():
    assert H_T * (-(-W_T // 4)) == ITEMS["tissue_plane"]
    image = edge_image(H_T, W_T, 237, 11, seed=70)
    want = TS.plane_of(image, 237, 11)
    assert (want == 0).any() and (want == 255).any()
    di = dev(image)
    pitch = -(-W_T // 4) * 4

    def run():  # the entry point itself, on a sentinel-filled plane (predict.tissue_plane allocates its own)
        plane = torch.full((H_T, pitch), 77, dtype=torch.uint8, device=DEV)
        K.call("selunet_tissue_plane", K.ptr(di), H_T, W_T, 237, 11, K.ptr(plane), pitch, K.stream_ptr())
        return {"plane": plane}

    got = under_grids(run)["plane"]
    assert np.array_equal(got[:, :W_T], want) and not got[:, W_T:].any()  # the whole pitched plane: padding bytes 0


def test_tissue_class_counts():
    assert H_T * (-(-W_T // 4)) == ITEMS["tissue_class_counts"]
    rng = np.random.Generator(np.random.PCG64(139))
    mask = rng.choice(np.array([0, 127, 255], np.uint8), (H_T, W_T), p=[0.5, 0.2, 0.3])
    plane = rng.choice(np.array([0, 255], np.uint8), (H_T, W_T))
    want = TR.counts_of(mask[plane != 0])
    forms = [(dev(mask), dev(plane)), (pitched(mask, 141), pitched(plane, 144))]

    def run():
        res = {}
        for i, (m, p) in enumerate(forms):
            acc = torch.zeros(4, dtype=torch.int64, device=DEV)
            PR.tissue_class_counts(m, p, acc)
            res[f"once{i}"] = acc.clone()
            PR.tissue_class_counts(m, p, acc)
            res[f"twice{i}"] = acc
        return res

    got = under_grids(run)
    for i in range(2):
        assert got[f"once{i}"].tolist() == want and got[f"twice{i}"].tolist() == [2 * v for v in want]


@pytest.mark.parametrize("connectivity", [8, 4])
def test_regions_label_and_apply_on_an_unaligned_width(connectivity):
    """70 x 139 (2 x 3 tiles, W % 4 = 3) against the flood fill: labels, then remove / fill / keep by row and the
    four counts; and the count-only form (labels NULL)."""
    assert H_T * (-(-W_T // 4)) == ITEMS["regions_apply"] == ITEMS["regions_flatten"]
    mask = RR.blobs(H_T, W_T, 7)
    want = RR.label(mask, 255, connectivity)
    names = np.unique(want[want > 0])
    action = (np.arange(len(names)) % 3).astype(np.uint8)
    act = np.where(want > 0, action[np.searchsorted(names, want)], 0)
    want_mask = np.where(act == 1, 0, mask).astype(np.uint8)  # (action 2 on a 255-region changes nothing)
    assert len(names) >= 3 and (want_mask != mask).any()
    da = dev(action)

    def run():
        m = pitched(mask, 141)
        lab = label_filled(m, 255, connectivity)  # sentinel-filled planes, whole pitched planes written
        counts = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
        PR._apply("test", m, None, None, counts[0])
        PR._apply("test", m, lab, da, counts[1])
        return {"labels": lab.labels[:, :W_T].contiguous(), "err": lab.err, "roots": lab.label_col, "mask": m.contiguous(),
                "counts": counts}

    got = under_grids(run)
    assert np.array_equal(got["labels"], want) and int(got["err"][0]) == 0 and np.array_equal(got["roots"], names)
    assert np.array_equal(got["mask"], want_mask)
    assert got["counts"].tolist() == [RR.counts(mask), RR.counts(want_mask)]


# ----------------------------------------------------------------------------- boundary.hip
def boundary_case(n, h, w, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    tgt = (blobs(n, h, w, seed + 1, waves=1.0) > 0.2).astype(F32)
    out = blobs(n, h, w, seed + 2, waves=2.0) + (tgt - 0.5) * 1.5
    sel = blobs(n, h, w, seed + 3) + F32(0.3)
    out.reshape(-1)[rng.choice(out.size, 6, replace=False)] = np.array([np.nan, np.inf, -np.inf, T_OUT, np.nan, T_OUT], F32)
    sel.reshape(-1)[rng.choice(out.size, 8, replace=False)] = np.array([np.nan, F32(0.1)] * 4, F32)
    tgt.reshape(-1)[rng.choice(out.size, 4, replace=False)] = np.array([2, 255, 2, 3], F32)
    d2t = np.stack([BR.separable_d2(BR.foreground(tgt[i], 0.5)) for i in range(n)])
    d2p = np.stack([BR.separable_d2(BR.foreground(out[i], T_OUT)) for i in range(n)])
    return out, sel, tgt, d2t, d2p


@pytest.mark.parametrize("selective", [True, False])
def test_boundary_bands_and_rows(selective):
    """Two images of 97 x 101 (hw % 4 = 1: the scalar tail; hw / 4 = 2449 items per image for the rows, 4899 for the
    bands of the batch): bins and rows equal the numpy oracle; two calls add (the rows' two maxima stay)."""
    n, h, w = 2, 97, 101
    hw = h * w
    assert (hw // 4, n * hw // 4 + 1) == (ITEMS["boundary_rows"], ITEMS["boundary_bands"])
    out, sel, tgt, d2t, d2p = boundary_case(n, h, w, 60)
    t_sel = F32(0.1)
    s = sel if selective else None
    r2 = MT.band_edges_sq([1, 2, 4, 8, 16]).astype(np.int64)
    flat = lambda a: None if a is None else a.reshape(n, -1)  # noqa: E731
    want_bins = BR.numpy_bands(out.ravel(), None if s is None else s.ravel(), tgt.ravel(), d2t.ravel(), r2, T_OUT, t_sel)
    want_rows = BR.numpy_rows(flat(out), flat(s), flat(tgt), flat(d2t), flat(d2p), T_OUT, t_sel, 4)
    assert (want_bins[:, 5] > 0).sum() >= len(r2) and want_rows[:, 4:].min() > 0
    o, sd, t = dev(out), dev(s), dev(tgt)
    a, b = dev(d2t.astype(np.int32)), dev(d2p.astype(np.int32))
    r2c = (K.c_int32 * len(r2))(*[int(v) for v in r2])

    def run():
        bins = torch.zeros(2, len(r2) + 2, 6, dtype=torch.int64, device=DEV)
        rows = torch.zeros(2, n, 6, dtype=torch.int64, device=DEV)
        for calls in (1, 2):
            for _ in range(calls):
                K.call("selunet_boundary_bands", K.ptr(o), K.ptr(sd), K.ptr(t), K.ptr(a), n, hw, float(T_OUT),
                       float(t_sel), r2c, len(r2), K.ptr(bins[calls - 1]), K.stream_ptr())
                K.call("selunet_boundary_rows", K.ptr(o), K.ptr(sd), K.ptr(t), K.ptr(a), K.ptr(b), n, hw, float(T_OUT),
                       float(t_sel), 4, K.ptr(rows[calls - 1]), K.stream_ptr())
        return {"bins": bins, "rows": rows}

    got = under_grids(run)
    assert np.array_equal(got["bins"][0], want_bins) and np.array_equal(got["bins"][1], 2 * want_bins)
    assert np.array_equal(got["rows"][0], want_rows)
    assert np.array_equal(got["rows"][1][:, :2], want_rows[:, :2]) and np.array_equal(got["rows"][1][:, 2:], 2 * want_rows[:, 2:])
