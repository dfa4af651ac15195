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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--halo", type=int, default=PR.HALO_MIN)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--compute_dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--fp32_path", default="exact", choices=["exact", "split"])
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
