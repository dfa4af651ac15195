"""Time whole-image prediction on one synthetic 4096 x 4096 image, stage by stage, beside what a user of the
package had to do before `predict_image` existed — measurement tool.

    python tools/predict_bench.py [--size 4096] [--tile 512] [--batch 16] [--rounds 3] > profiles/predict_tiles.txt
    python tools/predict_bench.py --fp32_path split >> profiles/predict_tiles.txt

(A) `predict_image`'s loop restated around HIP events: per batch of tiles selunet_tile_gather, the eval-mode
    forward of a selective UNet_B, selunet_tile_stitch; then the final copy of the mask and the probability map
    to the host. The sums over the batches of one pass are reported, the share of gather + stitch in the batch
    time, and the rate of `predict_image` itself (upload to final copy, host clock around a synchronise).
(B) The same image the old way: non-overlapping `tile` x `tile` numpy crops (no halo, so the seams are not
    those of a whole-image forward, and fewer pixels go through the network: (size / tile)^2 patches against
    ceil(size / (tile - 112))^2 tiles), uploaded per batch, `data.prep_batch`, forward, both logit tensors
    copied back, eval.py's fp32 numpy sigmoid and `> cut_off` on the host. Host clock per stage, each stage
    ending in a synchronise.
With `--tta` the tool times test-time augmentation instead (`... --tta > profiles/predict_tta.txt`,
`... --tta --fp32_path split >> profiles/predict_tta.txt`): passes of `none` (pass (A) above), `flips` and `d4`
(`predict_image`'s TTA loop restated around HIP events: transpose, flipped gather, forward, accumulate, finalize)
alternate with (C), what a user does for `d4` without it: 8 plain `predict_image` calls on numpy-transformed
copies, both planes to the host, un-flipped and averaged there, thresholds, `prob8` and counts in numpy (host
clock per stage). Reported per mode: the pass, its ratio to K x the `none` pass of the same run, the summed time
of the TTA-only kernels, their share of the pass and the bytes they move per second (bytes from the shapes).
With `--regions` the tool times region analysis instead (`... --regions > profiles/predict_regions.txt`,
`... --regions --fp32_path split >> profiles/predict_regions.txt`): (R) the stages of one labelling, its table and one
apply around HIP events (local, seam, flatten, the torch compaction of the roots, stats, apply), with the bytes they
move from the shapes, on the network's own mask and on adversarial masks (a serpentine and a full plane: one region
over every seam; noise at p = 0.59 and specks: very many); (P) `predict_image` with and without
`regions=True, min_region, fill_holes`, alternating, host clock; (H) the same tail done on the host with
scipy.ndimage and numpy on the planes of the same run, and whether both give the same mask and table.
With `--tissue` the tool times the tissue mask instead (`... --tissue > profiles/predict_tissue.txt`):
`predict_image(..., tissue=True)`'s loop restated around HIP events (tissue plane, window counts, the one read of the
counts, gather, forward and stitch of the kept tiles, the stitch of constants for the skipped ones, the class counts
over the tissue), alternating with the same loop without the rule, (a) on the mosaic as it is (the overhead where
nothing is skipped) and (b) with its right half replaced by the reference's glass model (the speed-up beside the
share of tiles forwarded).
One warm-up pass, then `rounds` passes of (A) and (B) alternating; the median pass is reported with the
min-max spread. Before timing, (A)'s mask is checked against the thresholds applied to its own planes, and
(B)'s host mask against it away from the seams. Nothing here is a threshold: the tool records times.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import selectivenet_for_semantic_segmentation_binary_amd as S  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import data as D  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd.synthetic import make_patches  # noqa: E402


def mosaic(size, seed=0):
    """A size x size uint8 RGB image: a mosaic of synthetic 256 x 256 patches."""
    k = -(-size // 256)
    p, _ = make_patches(k * k, 256, seed)
    return np.ascontiguousarray(p.reshape(k, k, 256, 256, 3).transpose(0, 2, 1, 3, 4).reshape(k * 256, k * 256, 3)[:size, :size])


def staged_pass(net, image, plan, batch, t_out, t_sel, dev):
    """One pass of predict_image's loop with an event after every stage: ({stage: ms}, mask, prob8, planes)."""
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    marks = []
    with torch.no_grad():
        t0 = ev()
        t0.record()
        img = torch.from_numpy(image).to(dev)
        origins = torch.from_numpy(plan.origins).to(dev)
        logit = torch.empty(plan.Hc, plan.Wc, device=dev)
        selp = torch.empty_like(logit)
        mask = torch.empty(plan.Hc, plan.Wc, dtype=torch.uint8, device=dev)
        prob = torch.empty_like(mask)
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        x_buf = torch.empty(min(batch, plan.n), 3, plan.tile, plan.tile, device=dev)
        t1 = ev()
        t1.record()
        for a in range(0, plan.n, batch):
            b = min(a + batch, plan.n)
            e = [ev() for _ in range(4)]
            e[0].record()
            x = PR.tile_gather(img, origins[a:b], plan.tile, plan.tile, "RGB", out=x_buf[:b - a])
            e[1].record()
            out, sel, _ = net(x)
            e[2].record()
            PR.tile_stitch(out, sel, plan.origins[a:b], origins[a:b], plan.halo, plan.H, plan.W, t_out, t_sel, logit,
                           selp, mask, prob, counts)
            e[3].record()
            marks.append(e)
        t2 = ev()
        t2.record()
        m, p = mask[:plan.H, :plan.W].cpu(), prob[:plan.H, :plan.W].cpu()
        c = counts.cpu()
        t3 = ev()
        t3.record()
        torch.cuda.synchronize()
    ms = {"upload": t0.elapsed_time(t1), "gather": sum(e[0].elapsed_time(e[1]) for e in marks),
          "forward": sum(e[1].elapsed_time(e[2]) for e in marks), "stitch": sum(e[2].elapsed_time(e[3]) for e in marks),
          "final copy": t2.elapsed_time(t3), "whole pass": t0.elapsed_time(t3)}
    return ms, m.numpy(), p.numpy(), (logit[:plan.H, :plan.W], selp[:plan.H, :plan.W]), c.numpy()


def old_way(net, image, tile, batch, cut_off, dev):
    """({stage: ms}, host mask): crops, prep_batch, forward, logits back, thresholds on the host."""
    H, W = image.shape[:2]
    ms = dict.fromkeys(("numpy crops", "upload + prep_batch", "forward", "logits to host", "host thresholds"), 0.0)
    mask = np.zeros((H, W), np.uint8)
    boxes = [(y, x) for y in range(0, H - tile + 1, tile) for x in range(0, W - tile + 1, tile)]

    def lap(name, t):
        torch.cuda.synchronize()
        now = time.perf_counter()
        ms[name] += (now - t) * 1e3
        return now

    t_all = time.perf_counter()
    with torch.no_grad():
        for a in range(0, len(boxes), batch):
            part = boxes[a:a + batch]
            t = time.perf_counter()
            crops = np.stack([image[y:y + tile, x:x + tile] for y, x in part])
            labels = np.zeros(crops.shape[:3], np.uint8)
            t = lap("numpy crops", t)
            x, _ = D.prep_batch(torch.from_numpy(crops).to(dev), torch.from_numpy(labels).to(dev), None, "RGB")
            t = lap("upload + prep_batch", t)
            out, sel, _ = net(x)
            t = lap("forward", t)
            o, s = out.cpu().numpy(), sel.cpu().numpy()
            t = lap("logits to host", t)
            with np.errstate(over="ignore"):  # eval.py:171,175,229-246: fp32 numpy sigmoid, then > cut_off
                pred = 1 / (1 + np.exp(-o)) > cut_off
                chosen = 1 / (1 + np.exp(-s)) > cut_off
            m = np.where(chosen, np.where(pred, 255, 0), 127).astype(np.uint8)
            for k, (y, x0) in enumerate(part):
                mask[y:y + tile, x0:x0 + tile] = m[k]
            t = lap("host thresholds", t)
    ms["whole pass"] = (time.perf_counter() - t_all) * 1e3
    return ms, mask


def tta_bytes(plan, members, selective=True):
    """The bytes the TTA-only kernels of one pass move, from the shapes: {stage: bytes}."""
    H, W, heads = plan.H, plan.W, 2 if selective else 1
    tiles = 0
    for c in range(members // 4):
        p = plan if c == 0 else PR.TilePlan(W, H, plan.tile, plan.halo)
        tiles += 4 * p.n
    px = H * W
    return {"transpose": 2 * 3 * px * (members // 8),
            "gather": tiles * plan.tile * plan.tile * (3 + 3 * 4),
            # per member and head: the core pixels inside the image read (4 B), the sum and the vote written
            # (4 + 1 B) and, but for the class's first member, read before (4 + 1 B)
            "accumulate": heads * px * (members * (4 + 5) + (members - members // 4) * 5),
            # per class and head 4 + 1 B read; the two mean planes, mask, prob8 and the two vote planes written
            "finalize": px * ((members // 4) * heads * 5 + heads * 5 + 2)}


def tta_pass(net, image, plan, batch, t_out, t_sel, dev, members):
    """One pass of predict_image(..., tta=) with an event after every stage: ({stage: ms}, planes, counts)."""
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    marks, tr = [], []
    H, W, tile, halo = plan.H, plan.W, plan.tile, plan.halo
    with torch.no_grad():
        t0 = ev()
        t0.record()
        img = torch.from_numpy(image).to(dev)
        x_buf = torch.empty(min(batch, plan.n), 3, tile, tile, device=dev)
        t1 = ev()
        t1.record()
        classes = []
        for c in range(members // 4):
            e = [ev(), ev()]
            e[0].record()
            src = PR.image_transpose(img) if c else img
            e[1].record()
            tr.append(e)
            h, w = int(src.shape[0]), int(src.shape[1])
            p = PR.TilePlan(h, w, tile, halo) if c else plan
            origins = torch.from_numpy(p.origins).to(dev)
            ws = -(-w // 8) * 8
            sums = [torch.zeros(h, ws, device=dev) for _ in range(2)]
            vts = [torch.zeros(h, ws, dtype=torch.uint8, device=dev) for _ in range(2)]
            for f in range(4):
                for a in range(0, p.n, batch):
                    b = min(a + batch, p.n)
                    e = [ev() for _ in range(4)]
                    e[0].record()
                    x = PR.tile_gather_flip(src, origins[a:b], tile, tile, "RGB", f, out=x_buf[:b - a])
                    e[1].record()
                    out, sel, _ = net(x)
                    e[2].record()
                    PR.tta_accumulate(out, sel, p.origins[a:b], origins[a:b], halo, f, f == 0, h, w, p.Hc, p.Wc, t_out,
                                      t_sel, sums[0], sums[1], vts[0], vts[1])
                    e[3].record()
                    marks.append(e)
            classes.append((sums[0], sums[1], vts[0], vts[1]))
        t2 = ev()
        t2.record()
        planes, counts = PR.tta_finalize(classes[0], classes[1] if members == 8 else None, members, H, W, t_out, t_sel)
        t3 = ev()
        t3.record()
        m, p8, v = planes[2][:, :W].cpu(), planes[3][:, :W].cpu(), planes[4][:, :W].cpu()
        c = counts.cpu()
        t4 = ev()
        t4.record()
        torch.cuda.synchronize()
    ms = {"upload": t0.elapsed_time(t1), "transpose": sum(e[0].elapsed_time(e[1]) for e in tr[1:]),
          "gather": sum(e[0].elapsed_time(e[1]) for e in marks), "forward": sum(e[1].elapsed_time(e[2]) for e in marks),
          "accumulate": sum(e[2].elapsed_time(e[3]) for e in marks), "finalize": t2.elapsed_time(t3),
          "final copy": t3.elapsed_time(t4), "whole pass": t0.elapsed_time(t4)}
    return ms, [t[:, :W] for t in planes], c.numpy()


def host_d4(net, image, tile, halo, batch, t_out, t_sel):
    """(C): `d4` by hand around today's predict_image. ({stage: ms}, mean logit, mask)."""
    ms = dict.fromkeys(("numpy transforms", "predict_image x 8", "planes to host", "un-flip + mean", "host thresholds"), 0.0)

    def lap(name, t):
        torch.cuda.synchronize()
        now = time.perf_counter()
        ms[name] += (now - t) * 1e3
        return now

    def turn(k, a):
        a = a.swapaxes(0, 1) if k & 4 else a
        a = a[::-1] if k & 2 else a
        return a[:, ::-1] if k & 1 else a

    def back(k, a):
        a = a[:, ::-1] if k & 1 else a
        a = a[::-1] if k & 2 else a
        return a.T if k & 4 else a

    t_all = t = time.perf_counter()
    acc = [[None, None], [None, None]]  # [class][head], in the image's orientation
    votes = 0
    for k in range(8):
        im = np.ascontiguousarray(turn(k, image))
        t = lap("numpy transforms", t)
        pred = PR.predict_image(net, im, tile=tile, halo=halo, batch_size=batch, prob8=False)
        t = lap("predict_image x 8", t)
        planes = [pred.logit.cpu().numpy(), pred.selection.cpu().numpy()]
        t = lap("planes to host", t)
        for i in range(2):
            m = back(k, planes[i])
            acc[k >> 2][i] = m.copy() if acc[k >> 2][i] is None else acc[k >> 2][i] + m
        votes = votes + (back(k, planes[0]) >= np.float32(t_out)).astype(np.uint8)
        t = lap("un-flip + mean", t)
    mean = [(acc[0][i] + acc[1][i]) * np.float32(0.125) for i in range(2)]
    t = lap("un-flip + mean", t)
    with np.errstate(over="ignore"):
        mask = np.where(~(mean[1] >= np.float32(t_sel)), 127, np.where(mean[0] >= np.float32(t_out), 255, 0)).astype(np.uint8)
        prob8 = np.floor(255.0 / (1.0 + np.exp(-mean[0])) + 0.5).astype(np.uint8)
        counts = [int((mask == 0).sum()), int((mask == 255).sum()), int((mask == 127).sum()), mask.size]
    t = lap("host thresholds", t)
    ms["whole pass"] = (time.perf_counter() - t_all) * 1e3
    return ms, mean[0], mask, votes, counts, prob8


def tta_report(a, net, image, plan, t_out, t_sel, dev, mpix):
    """--tta: passes of none, flips, d4 and the host-side d4 alternating; the report of the module docstring."""
    modes = {"none": 1, "flips": 4, "d4": 8}
    run = {"none": lambda: staged_pass(net, image, plan, a.batch, t_out, t_sel, dev)[0],
           "flips": lambda: tta_pass(net, image, plan, a.batch, t_out, t_sel, dev, 4)[0],
           "d4": lambda: tta_pass(net, image, plan, a.batch, t_out, t_sel, dev, 8)[0]}
    # ---- warm-up and checks: the restated loop against predict_image, and against the host-side mean
    ok = True
    for mode in ("flips", "d4"):
        _, planes, counts = tta_pass(net, image, plan, a.batch, t_out, t_sel, dev, modes[mode])
        pred = PR.predict_image(net, image, tile=a.tile, halo=a.halo, batch_size=a.batch, tta=mode)
        same = bool(torch.equal(planes[0], pred.logit)) and bool(torch.equal(planes[2], pred.mask)) and \
            bool(torch.equal(planes[4], pred.votes)) and counts.tolist() == pred.counts.tolist()
        print(f"({mode}) restated loop == predict_image(tta={mode!r}): {same}; counts "
              f"{dict(zip(PR.COUNT_NAMES, counts.tolist()))}, unanimous fraction {pred.unanimous_fraction:.4f}")
        ok = ok and same
    _, mean, mask, votes, hcounts, _ = host_d4(net, image, a.tile, a.halo, a.batch, t_out, t_sel)
    d = float(np.abs(mean - planes[0].cpu().numpy()).max())
    same = d == 0.0 and bool(np.array_equal(mask, planes[2].cpu().numpy())) and \
        bool(np.array_equal(votes, planes[4].cpu().numpy())) and hcounts == counts.tolist()
    print(f"(C) host-side d4 mean vs the device's: max |difference| {d}; mask, votes and counts equal: {same}")
    ok = ok and same
    run["none"]()
    # ---- timing
    ts = {m: [] for m in modes}
    tc = []
    for _ in range(a.rounds):
        for m in modes:
            ts[m].append(run[m]())
        tc.append(host_d4(net, image, a.tile, a.halo, a.batch, t_out, t_sel)[0])

    def row(rows, k):
        v = [t[k] for t in rows]
        return statistics.median(v), f"{statistics.median(v):10.2f} [{min(v):.2f} .. {max(v):.2f}]"

    none, s = row(ts["none"], "whole pass")
    v = [t["whole pass"] for t in ts["none"]]
    spread = (max(v) - min(v)) / none
    print("(none) pass (A): gather, forward, stitch (HIP events, summed over the batches of a pass)")
    for k in ("upload", "gather", "forward", "stitch", "final copy", "whole pass"):
        print(f"    {k:<22}{row(ts['none'], k)[1]}")
    print(f"    spread of the passes (max - min) / median: {spread:.4f}")
    for mode in ("flips", "d4"):
        K = modes[mode]
        by = tta_bytes(plan, K)
        print(f"({mode}) {K} members: transpose, flipped gather, forward, accumulate, finalize")
        med = {}
        for k in ("upload", "transpose", "gather", "forward", "accumulate", "finalize", "final copy", "whole pass"):
            med[k], s = row(ts[mode], k)
            gbs = f"  {by[k] / 1e6:9.1f} MB, {by[k] / med[k] / 1e6:7.1f} GB/s" if k in by and med[k] > 0 else ""
            print(f"    {k:<22}{s}{gbs}")
        only = sum(med[k] for k in by)
        print(f"    TTA-only kernels (transpose + gather + accumulate + finalize): {only:.2f} ms = {only / med['whole pass']:.4f} "
              f"of the pass, {sum(by.values()) / only / 1e6:.1f} GB/s over them")
        print(f"    whole pass / ({K} x the none pass): {med['whole pass'] / (K * none):.4f}; "
              f"{mpix / med['whole pass'] * 1e3:.1f} Mpixel/s")
    print("(C) d4 on the host: 8 x predict_image, planes to the host, numpy un-flip, mean, thresholds (host clock per stage)")
    for k in ("numpy transforms", "predict_image x 8", "planes to host", "un-flip + mean", "host thresholds", "whole pass"):
        m, s = row(tc, k)
        print(f"    {k:<22}{s}")
    print(f"    (C) / (d4) whole pass = {row(tc, 'whole pass')[0] / row(ts['d4'], 'whole pass')[0]:.2f}")
    print("checks passed:", ok)
    return 0 if ok else 1


# ----------------------------------------------------------------------------- --tissue
TISSUE_STAGES = ("upload", "tissue plane", "window counts", "read of the counts", "gather", "forward", "stitch",
                 "stitch of constants", "class counts", "final copy", "whole pass")


def tissue_pass(net, image, plan, batch, t_out, t_sel, dev, rule):
    """One pass of predict_image's loop, with the tissue rule (bright, spread, min_pixels) or without (None), with an
    event after every stage: ({stage: ms}, mask, kept | None, counts [8 | 4])."""
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    tile, halo, H, W = plan.tile, plan.halo, plan.H, plan.W
    marks, consts = [], []
    with torch.no_grad():
        t = [ev() for _ in range(8)]
        t[0].record()
        img = torch.from_numpy(image).to(dev)
        origins = torch.from_numpy(plan.origins).to(dev)
        t[1].record()
        keep = glass = None
        if rule:
            glass = PR.tissue_plane(img, rule[0], rule[1])
        t[2].record()
        if rule:
            window = PR.tile_tissue_counts(glass, origins, tile, tile)
        t[3].record()
        if rule:
            keep = window.cpu().numpy() >= rule[2]
        t[4].record()
        logit = torch.empty(plan.Hc, plan.Wc, device=dev)
        selp = torch.empty_like(logit)
        mask = torch.empty(plan.Hc, plan.Wc, dtype=torch.uint8, device=dev)
        prob = torch.empty_like(mask)
        counts = torch.zeros(8 if rule else 4, dtype=torch.int64, device=dev)
        run_host, run = PR._kept_origins(plan.origins, origins, keep)
        x_buf = torch.empty(min(batch, plan.n), 3, tile, tile, device=dev)
        for a in range(0, len(run_host), batch):
            b = min(a + batch, len(run_host))
            e = [ev() for _ in range(4)]
            e[0].record()
            x = PR.tile_gather(img, run[a:b], tile, tile, "RGB", out=x_buf[:b - a])
            e[1].record()
            out, sel, _ = net(x)
            e[2].record()
            PR.tile_stitch(out, sel, run_host[a:b], run[a:b], halo, H, W, t_out, t_sel, logit, selp, mask, prob, counts[:4])
            e[3].record()
            marks.append(e)
        if rule:
            for out, sel, oh, od in PR._Skipped(min(batch, plan.n), tile, True, dev).batches(plan.origins, keep):
                e = [ev(), ev()]
                e[0].record()
                PR.tile_stitch(out, sel, oh, od, halo, H, W, t_out, t_sel, logit, selp, mask, prob, counts[:4])
                e[1].record()
                consts.append(e)
        t[5].record()
        if rule:
            PR.tissue_class_counts(mask[:H, :W], glass, counts[4:])
        t[6].record()
        m, p = mask[:H, :W].cpu(), prob[:H, :W].cpu()
        c = counts.cpu()
        t[7].record()
        torch.cuda.synchronize()
    ms = {"upload": t[0].elapsed_time(t[1]), "tissue plane": t[1].elapsed_time(t[2]), "window counts": t[2].elapsed_time(t[3]),
          "read of the counts": t[3].elapsed_time(t[4]), "gather": sum(e[0].elapsed_time(e[1]) for e in marks),
          "forward": sum(e[1].elapsed_time(e[2]) for e in marks), "stitch": sum(e[2].elapsed_time(e[3]) for e in marks),
          "stitch of constants": sum(e[0].elapsed_time(e[1]) for e in consts), "class counts": t[5].elapsed_time(t[6]),
          "final copy": t[6].elapsed_time(t[7]), "whole pass": t[0].elapsed_time(t[7])}
    return ms, m.numpy(), keep, c.numpy()


def tissue_report(a, net, image, plan, t_out, t_sel, dev, mpix):
    """--tissue: the passes with and without the rule alternating, on the mosaic and on its half-glass version."""
    rule = (PR.TISSUE_BRIGHT, PR.TISSUE_SPREAD, 1)
    half = image.copy()
    rng = np.random.default_rng(1)
    half[:, a.size // 2:] = np.floor(255 * np.clip(0.96 + 0.005 * rng.standard_normal(half[:, a.size // 2:].shape), 0, 1) + 0.5)
    kw = dict(tile=a.tile, halo=a.halo, batch_size=a.batch)

    def row(rows, k):
        v = [t[k] for t in rows]
        return statistics.median(v), f"{statistics.median(v):10.3f} [{min(v):.3f} .. {max(v):.3f}]"

    ok = True
    for name, im in (("(a) the mosaic as it is", image), ("(b) the right half replaced by the glass model", half)):
        # ---- warm-up and checks: the restated loop against predict_image
        _, mask, keep, counts = tissue_pass(net, im, plan, a.batch, t_out, t_sel, dev, rule)
        tissue_pass(net, im, plan, a.batch, t_out, t_sel, dev, None)
        pred = PR.predict_image(net, im, tissue=True, **kw)
        same = bool(np.array_equal(pred.mask.cpu().numpy(), mask)) and bool(np.array_equal(pred.tiles_kept[0], keep)) and \
            counts[:4].tolist() == pred.counts.tolist() and counts[4:].tolist() == pred.tissue_counts.tolist()
        ok = ok and same
        off = PR.predict_image(net, im, **kw)
        cover = torch.from_numpy(np.kron(keep.reshape(plan.grid), np.ones((plan.core, plan.core), bool))[:plan.H, :plan.W]).to(dev)
        kept_equal = bool(torch.equal(pred.logit[cover], off.logit[cover])) and bool(torch.equal(pred.mask[cover], off.mask[cover]))
        ok = ok and kept_equal
        kept_n = int(keep.sum())
        print(f"{name}: tissue pixels {int(pred.tissue_counts[3])} of {plan.H * plan.W} "
              f"({int(pred.tissue_counts[3]) / (plan.H * plan.W):.4f}); tiles forwarded {kept_n} of {plan.n} "
              f"({kept_n / plan.n:.4f}) in {-(-kept_n // a.batch)} batches (the last of {kept_n % a.batch or a.batch}); "
              f"{plan.n - kept_n} skipped")
        print(f"    restated loop == predict_image(tissue=True): {same}; kept pixels bit-equal to tissue=False: {kept_equal}")
        print(f"    counts {dict(zip(PR.COUNT_NAMES, pred.counts.tolist()))}; over tissue "
              f"{dict(zip(PR.COUNT_NAMES, pred.tissue_counts.tolist()))}; tumor fraction of selected {pred.tumor_fraction:.4f}, "
              f"of tissue {pred.tumor_fraction_of_tissue:.4f}")
        # ---- timing: without and with the rule, alternating in one process
        t_off, t_on, h_off, h_on = [], [], [], []
        for _ in range(a.rounds):
            t_off.append(tissue_pass(net, im, plan, a.batch, t_out, t_sel, dev, None)[0])
            t_on.append(tissue_pass(net, im, plan, a.batch, t_out, t_sel, dev, rule)[0])
            for extra, into in ((dict(), h_off), (dict(tissue=True), h_on)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                p = PR.predict_image(net, im, **kw, **extra)
                p.mask.cpu(), p.prob8.cpu()
                torch.cuda.synchronize()
                into.append((time.perf_counter() - t) * 1e3)
        print(f"    {'stage (HIP events)':<24}{'tissue=False':>34}{'tissue=True':>34}")
        med = {}
        for k in TISSUE_STAGES:
            (m0, s0), (m1, s1) = row(t_off, k), row(t_on, k)
            med[k] = (m0, m1)
            print(f"    {k:<24}{s0:>34}{s1:>34}")
        new = sum(med[k][1] for k in ("tissue plane", "window counts", "class counts"))
        gs = med["gather"][1] + med["stitch"][1] + med["stitch of constants"][1]
        px = plan.H * plan.W
        moved = px * 3 + px + 1.6 * px + 2 * px  # plane: 3 B in, 1 B out; window counts: about 1.6 x the plane; class counts: mask + plane
        print(f"    new launches (plane + window counts + class counts): {new:.3f} ms ({moved / 1e6:.1f} MB from the shapes, "
              f"{moved / new / 1e6:.1f} GB/s); gather + stitch (+ constants) of the same pass: {gs:.3f} ms; the one extra read: "
              f"{med['read of the counts'][1]:.3f} ms")
        ratio = med["whole pass"][1] / med["whole pass"][0]
        print(f"    whole pass tissue=True / tissue=False: {ratio:.4f} (forwarded / total tiles {kept_n / plan.n:.4f}); forward "
              f"{med['forward'][1] / med['forward'][0]:.4f}; {mpix / med['whole pass'][1] * 1e3:.1f} against "
              f"{mpix / med['whole pass'][0] * 1e3:.1f} Mpixel/s")
        m0, m1 = statistics.median(h_off), statistics.median(h_on)
        print(f"    predict_image + mask and prob8 to the host (host clock): {m0:.2f} [{min(h_off):.2f} .. {max(h_off):.2f}] without, "
              f"{m1:.2f} [{min(h_on):.2f} .. {max(h_on):.2f}] with the rule: ratio {m1 / m0:.4f}")
    print("checks passed:", ok)
    return 0 if ok else 1


# ----------------------------------------------------------------------------- --regions
REGION_STAGES = ("local", "seam", "flatten", "roots to rows (torch)", "stats", "action (torch)", "apply")


def region_bytes(H, W):
    """Algorithmic bytes per stage, from the shapes: mask 1 B, parent / label 4 B, root flag 1 B, prob8 1 B a pixel;
    the seam pass touches about three 4-B words per pixel of the tile borders."""
    px, seam = H * W, (-(-H // 64) - 1) * W + (-(-W // 64) - 1) * H
    return {"local": px * (1 + 4), "seam": seam * 3 * 4, "flatten": px * (4 + 4 + 1), "stats": px * (4 + 1 + 1),
            "apply": px * (1 + 4 + 1)}


def region_stages(mask, prob8, value, connectivity, min_region):
    """One labelling of `mask`, its table, and one apply (regions below min_region -> 0, on a copy) with an event
    after every stage: ({stage: ms}, Regions, error word)."""
    from selectivenet_for_semantic_segmentation_binary_amd import _lib as K

    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    H, W = mask.shape
    lp, dev = -(-W // 4) * 4, mask.device
    parent = torch.empty(H, lp, dtype=torch.int32, device=dev)
    labels = torch.empty(H, lp, dtype=torch.int32, device=dev)
    roots = torch.empty(H, lp, dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    work, counts = mask.clone(), torch.zeros(4, dtype=torch.int64, device=dev)
    e = [ev() for _ in range(len(REGION_STAGES) + 1)]
    e[0].record()
    for i, passes in enumerate((1, 2, 4)):
        K.call("selunet_regions_label", K.ptr(mask), mask.stride(0), H, W, value, connectivity, K.ptr(parent),
               K.ptr(labels), K.ptr(roots), lp, K.ptr(err), passes, K.stream_ptr())
        e[i + 1].record()
    pos = torch.nonzero(roots.view(-1)).view(-1)
    parent.view(-1)[pos] = torch.arange(pos.numel(), dtype=torch.int32, device=dev)
    lab = PR._Labelling(H, W, lp, labels, parent, lp, 1 + torch.div(pos, lp, rounding_mode="floor") * W + pos % lp, err)
    e[4].record()
    reg = PR._table("predict_bench", mask, lab, prob8)
    e[5].record()
    action = (reg.area < min_region).to(torch.uint8)
    e[6].record()
    if lab.n:
        PR._apply("predict_bench", work, lab, action, counts)
    e[7].record()
    torch.cuda.synchronize()
    return {k: e[i].elapsed_time(e[i + 1]) for i, k in enumerate(REGION_STAGES)}, reg, int(err.item())


def host_regions(mask_t, prob_t, min_region, fill_holes):
    """What a user does without the feature: mask and prob8 to the host, scipy.ndimage for the labels and the
    table, the two clean-up steps in numpy. ({stage: ms}, final mask, table {column: int64 [n]} by canonical label)."""
    from scipy import ndimage

    ms = dict.fromkeys(("planes to host", "ndimage.label x 3", "tables (find_objects / sum / minimum)", "clean-up (numpy)"), 0.0)

    def lap(name, t):
        torch.cuda.synchronize()
        now = time.perf_counter()
        ms[name] += (now - t) * 1e3
        return now

    def table(mask, lab, n, prob8=None, full=True):
        idx = np.arange(1, n + 1)
        H, W = mask.shape
        box = ndimage.find_objects(lab)
        t = {"area": np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int64),
             "y_min": np.array([b[0].start for b in box], np.int64), "x_min": np.array([b[1].start for b in box], np.int64),
             "y_max": np.array([b[0].stop - 1 for b in box], np.int64), "x_max": np.array([b[1].stop - 1 for b in box], np.int64)}
        ab = np.pad(mask == 127, 1)
        near = ab[:-2, 1:-1].astype(np.uint8) + ab[2:, 1:-1] + ab[1:-1, :-2] + ab[1:-1, 2:]
        t["abstain_contacts"] = np.asarray(ndimage.sum(near, lab, idx)).astype(np.int64).reshape(n)
        if full:  # sums of coordinates below 2^53: exact in the float64 that ndimage.sum returns
            yy, xx = np.indices((H, W), dtype=np.int32, sparse=True)
            t["sum_y"] = np.asarray(ndimage.sum(np.broadcast_to(yy, (H, W)), lab, idx)).astype(np.int64).reshape(n)
            t["sum_x"] = np.asarray(ndimage.sum(np.broadcast_to(xx, (H, W)), lab, idx)).astype(np.int64).reshape(n)
            t["prob_sum"] = np.asarray(ndimage.sum(prob8, lab, idx)).astype(np.int64).reshape(n)
            first = np.asarray(ndimage.minimum(np.arange(H * W, dtype=np.int64).reshape(H, W), lab, idx)).reshape(n)
            t["label"] = 1 + first.astype(np.int64)
        return t

    t_all = t = time.perf_counter()
    mask, prob8 = mask_t.cpu().numpy().copy(), prob_t.cpu().numpy()
    t = lap("planes to host", t)
    eight = np.ones((3, 3), int)
    if min_region > 0:
        lab, n = ndimage.label(mask == 255, structure=eight)
        t = lap("ndimage.label x 3", t)
        tb = table(mask, lab, n, full=False)
        t = lap("tables (find_objects / sum / minimum)", t)
        mask[np.concatenate([[False], tb["area"] < min_region])[lab]] = 0
        t = lap("clean-up (numpy)", t)
    if fill_holes > 0:
        H, W = mask.shape
        lab, n = ndimage.label(mask == 0)
        t = lap("ndimage.label x 3", t)
        tb = table(mask, lab, n, full=False)
        t = lap("tables (find_objects / sum / minimum)", t)
        hole = ((tb["y_min"] > 0) & (tb["x_min"] > 0) & (tb["y_max"] < H - 1) & (tb["x_max"] < W - 1)
                & (tb["abstain_contacts"] == 0) & (tb["area"] <= fill_holes))
        mask[np.concatenate([[False], hole])[lab]] = 255
        t = lap("clean-up (numpy)", t)
    lab, n = ndimage.label(mask == 255, structure=eight)
    t = lap("ndimage.label x 3", t)
    tb = table(mask, lab, n, prob8)
    order = np.argsort(tb["label"])
    tb = {k: v[order] for k, v in tb.items()}
    t = lap("tables (find_objects / sum / minimum)", t)
    ms["whole tail"] = (time.perf_counter() - t_all) * 1e3
    return ms, mask, tb


def regions_report(a, net, image, plan, t_out, t_sel, dev, mpix):
    """--regions: per-stage times on the network's own mask and on two adversarial masks; the clean-up's share of a
    pass, alternating with the plain pass; and the host-side alternative on the same planes."""
    H = W = a.size
    kw = dict(tile=a.tile, halo=a.halo, batch_size=a.batch)
    clean = dict(min_region=a.min_region, fill_holes=a.fill_holes)
    plain = PR.predict_image(net, image, **kw)
    serp = np.zeros((H, W), np.uint8)
    serp[0::2] = 255
    for k, y in enumerate(range(1, H - 1, 2)):
        serp[y, W - 1 if k % 2 == 0 else 0] = 255
    noise = ((np.random.Generator(np.random.PCG64(59)).random((H, W)) < 0.59) * 255).astype(np.uint8)
    speck = ((np.random.Generator(np.random.PCG64(5)).random((H, W)) < 0.05) * 255).astype(np.uint8)
    masks = [("the network's mask, 8-connected", plain.mask, 8),
             ("serpentine over the whole image (one region), 4-connected", torch.from_numpy(serp).to(dev), 4),
             ("all 255 (one region), 8-connected", torch.full((H, W), 255, dtype=torch.uint8, device=dev), 8),
             ("noise p = 0.59, 4-connected", torch.from_numpy(noise).to(dev), 4),
             ("specks p = 0.05, 8-connected", torch.from_numpy(speck).to(dev), 8)]
    by = region_bytes(H, W)

    def row(rows, k):
        v = [t[k] for t in rows]
        return statistics.median(v), f"{statistics.median(v):10.3f} [{min(v):.3f} .. {max(v):.3f}]"

    ok = True
    for name, m, conn in masks:
        region_stages(m, plain.prob8, 255, conn, a.min_region)  # warm-up
        runs = [region_stages(m, plain.prob8, 255, conn, a.min_region) for _ in range(a.rounds)]
        reg = runs[0][1]
        ok = ok and all(r[2] == 0 for r in runs)
        big = int(reg.area.max().item()) if len(reg) else 0
        print(f"(R) stages on {name}: {len(reg)} regions, the largest of {big} pixels; error word {runs[0][2]}")
        total = 0.0
        for k in REGION_STAGES:
            med, s = row([r[0] for r in runs], k)
            total += med
            gbs = f"  {by[k] / 1e6:8.1f} MB, {by[k] / med / 1e6:7.1f} GB/s" if k in by and med > 0 else ""
            print(f"    {k:<24}{s}{gbs}")
        print(f"    {'sum of the stages':<24}{total:10.3f}")
    # ---- clean_mask as predict_image runs it (three labellings, their tables, two applies, the counts), HIP events
    tc = []
    for _ in range(a.rounds + 1):
        work = plain.mask.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        PR.clean_mask(work, plain.prob8, **clean)
        e1.record()
        torch.cuda.synchronize()
        tc.append(e0.elapsed_time(e1))
    tc = tc[1:]
    print(f"(R) clean_mask(min_region={a.min_region}, fill_holes={a.fill_holes}) on the network's mask, first call to the "
          f"one read: {statistics.median(tc):10.3f} [{min(tc):.3f} .. {max(tc):.3f}]")
    # ---- the share of a pass: plain and with the clean-up, alternating, host clock around a synchronise
    def timed(**extra):
        torch.cuda.synchronize()
        t = time.perf_counter()
        pred = PR.predict_image(net, image, **kw, **extra)
        pred.mask.cpu(), pred.prob8.cpu()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, pred

    timed(regions=True, **clean)
    tp, tr, th = [], [], []
    for _ in range(a.rounds):
        tp.append(timed()[0])
        ms, pred = timed(regions=True, **clean)
        tr.append(ms)
        th.append(host_regions(plain.mask, plain.prob8, a.min_region, a.fill_holes)[0])
    mp, mr = statistics.median(tp), statistics.median(tr)
    print(f"(P) predict_image + mask and prob8 to the host, plain:        {mp:10.2f} [{min(tp):.2f} .. {max(tp):.2f}]")
    print(f"(P) the same with regions=True, min_region={a.min_region}, fill_holes={a.fill_holes}: {mr:10.2f} "
          f"[{min(tr):.2f} .. {max(tr):.2f}]: + {mr - mp:.2f} ms = {(mr - mp) / mp:.4f} of the plain pass; "
          f"{len(pred.regions)} regions, {pred.cleanup}")
    print("(H) the same tail on the host: planes to the host, scipy.ndimage, numpy (host clock per stage)")
    for k in th[0]:
        print(f"    {k:<40}{row(th, k)[1]}")
    print(f"    (H) whole tail / (P) added time = {row(th, 'whole tail')[0] / max(mr - mp, 1e-9):.1f}")
    _, host_mask, host_table = host_regions(plain.mask, plain.prob8, a.min_region, a.fill_holes)
    dev_table = pred.regions.numpy()
    same = bool(np.array_equal(host_mask, pred.mask.cpu().numpy())) and \
        all(np.array_equal(dev_table[c], host_table[c]) for c in PR.REGION_COLUMNS)
    print(f"(H) host mask and table equal the device's, every column: {same}")
    print("checks passed:", ok and same)
    return 0 if ok and same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--halo", type=int, default=PR.HALO_MIN)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--compute_dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--fp32_path", default="exact", choices=["exact", "split"])
    ap.add_argument("--tta", action="store_true", help="time test-time augmentation: none, flips, d4 and d4 on the host")
    ap.add_argument("--regions", action="store_true", help="time region labelling, the table and the clean-up")
    ap.add_argument("--tissue", action="store_true", help="time the tissue mask: overhead where nothing is skipped, speed-up on a half-glass image")
    ap.add_argument("--min_region", type=int, default=64)
    ap.add_argument("--fill_holes", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("predict_bench: no GPU visible (timings are taken on the device only)")
    if a.size % a.tile:
        sys.exit("predict_bench: the old way cuts whole patches: --size must be a multiple of --tile")
    dev = torch.device("cuda", 0)
    image = mosaic(a.size)
    dt = torch.bfloat16 if a.compute_dtype == "bf16" else torch.float32
    torch.manual_seed(0)
    net = S.UNet_B("RGB", selective=True, compute_dtype=dt, fp32_eval_path=a.fp32_path).to(dev).train(False)
    plan = PR.TilePlan(a.size, a.size, a.tile, a.halo)
    with torch.no_grad():  # spread a fresh network's heads around their thresholds: all three mask classes occur
        net.conv1x1.weight.mul_(64)
        net.conv_select.weight.mul_(64)
        x = PR.tile_gather(torch.from_numpy(image).to(dev), torch.tensor([[a.tile, a.tile]], dtype=torch.int32, device=dev),
                           a.tile, a.tile)
        out, sel, _ = net(x)
        net.conv1x1.bias.sub_(out.median())
        net.conv_select.bias.sub_(sel.median() + 0.5 * sel.std())
    t_out = t_sel = MT.logit_threshold("eval", 0.5)
    mpix = a.size * a.size / 1e6
    print(f"{torch.cuda.get_device_name(0)}; {a.size} x {a.size} image ({mpix:.1f} Mpixel), selective UNet_B "
          f"{a.compute_dtype} ({a.fp32_path}), batch {a.batch}; median of {a.rounds} passes [min .. max], ms")
    print(f"(A) {plan!r}: {plan.n} tiles in {-(-plan.n // a.batch)} batches")
    if a.tta:
        return tta_report(a, net, image, plan, t_out, t_sel, dev, mpix)
    if a.tissue:
        return tissue_report(a, net, image, plan, t_out, t_sel, dev, mpix)
    if a.regions:
        return regions_report(a, net, image, plan, t_out, t_sel, dev, mpix)
    n_old = (a.size // a.tile) ** 2
    print(f"(B) {n_old} patches of {a.tile} x {a.tile} without halo in {-(-n_old // a.batch)} batches")

    # ---- warm-up and checks
    ms, mask, prob, (logit, selp), counts = staged_pass(net, image, plan, a.batch, t_out, t_sel, dev)
    lo, se = logit.cpu().numpy(), selp.cpu().numpy()
    want = np.where(~(se >= np.float32(t_sel)), 127, np.where(lo >= np.float32(t_out), 255, 0)).astype(np.uint8)
    ok = bool(np.array_equal(mask, want)) and int(counts[3]) == a.size * a.size and int(counts[:3].sum()) == int(counts[3])
    _, old_mask = old_way(net, image, a.tile, a.batch, 0.5, dev)
    inner = np.ones(mask.shape, bool)  # pixels further than 56 from a seam of (B) and from the image's edge
    for k in range(0, a.size + 1, a.tile):
        inner[max(k - 56, 0):k + 56] = False
        inner[:, max(k - 56, 0):k + 56] = False
    differ = int((old_mask[inner] != mask[inner]).sum())
    print(f"(A) mask == thresholds on its planes, counts consistent: {ok}; counts {dict(zip(PR.COUNT_NAMES, counts.tolist()))}")
    print(f"(B) host mask differs from (A) on {differ} of {int(inner.sum())} pixels further than 56 from a seam or an edge, "
          f"on {int((old_mask != mask).sum())} of {mask.size} overall")
    pred = PR.predict_image(net, image, tile=a.tile, halo=a.halo, batch_size=a.batch)
    ok = ok and bool(np.array_equal(pred.mask.cpu().numpy(), mask)) and pred.counts.tolist() == counts.tolist()

    # ---- timing
    ta, tb, tp = [], [], []
    for _ in range(a.rounds):
        ta.append(staged_pass(net, image, plan, a.batch, t_out, t_sel, dev)[0])
        tb.append(old_way(net, image, a.tile, a.batch, 0.5, dev)[0])
        torch.cuda.synchronize()
        t = time.perf_counter()
        pred = PR.predict_image(net, image, tile=a.tile, halo=a.halo, batch_size=a.batch)
        pred.mask.cpu(), pred.prob8.cpu()
        torch.cuda.synchronize()
        tp.append((time.perf_counter() - t) * 1e3)

    def row(ts, k):
        v = [t[k] for t in ts]
        return statistics.median(v), f"{statistics.median(v):10.2f} [{min(v):.2f} .. {max(v):.2f}]"

    print("(A) tiles gathered and stitched on the device (HIP events, summed over the batches of a pass)")
    med = {}
    for k in ("upload", "gather", "forward", "stitch", "final copy", "whole pass"):
        med[k], s = row(ta, k)
        print(f"    {k:<22}{s}")
    batch_ms = med["gather"] + med["forward"] + med["stitch"]
    print(f"    gather + stitch share of the batch time: {(med['gather'] + med['stitch']) / batch_ms:.4f}")
    print(f"    whole pass: {mpix / med['whole pass'] * 1e3:.1f} Mpixel/s")
    mp = statistics.median(tp)
    print(f"    predict_image + mask and prob8 to the host (host clock): {mp:10.2f} [{min(tp):.2f} .. {max(tp):.2f}] "
          f"= {mpix / mp * 1e3:.1f} Mpixel/s")
    print("(B) numpy crops, prep_batch, forward, logits to the host, thresholds there (host clock per stage)")
    for k in ("numpy crops", "upload + prep_batch", "forward", "logits to host", "host thresholds", "whole pass"):
        m, s = row(tb, k)
        med[k + " B"] = m
        print(f"    {k:<22}{s}")
    print(f"    whole pass: {mpix / med['whole pass B'] * 1e3:.1f} Mpixel/s; (B) / (A) whole pass = "
          f"{med['whole pass B'] / med['whole pass']:.2f}")
    print("checks passed:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
