"""Time the per-patch report's two calls (selunet_seg_metrics_rows, selunet_patch_auc) on one eval batch,
beside the eval-mode forward of the same batch in the same run — measurement tool.

    python tools/patch_report_bench.py [--iters 200] [--rounds 5] > profiles/patch_report.txt

Per batch shape (16 x 256 x 256 and 8 x 512 x 512 fp32 logits), without and with selection logits:
  (a) one selunet_seg_metrics call over the batch (what eval already pays),
  (b) one selunet_seg_metrics_rows call, (c) one selunet_patch_auc call,
  (d) what `metrics.PatchReport.add_batch` enqueues for the batch (one memset and (b) + (c) over all
      pixels; with selection a second (b) + (c) over the selected ones),
  (e) the fp32 eval-mode forward of a selective UNet_B on a batch of that shape.
HIP events around `iters` back-to-back calls after a warm-up, the variants alternating over `rounds`
rounds; the median round is reported with the min-max spread. Logits ~ N(0, 1), 40 % label-1 pixels,
selection logits ~ N(0, 1) against the cut-off 0.5. Before timing, the rows are checked against
selunet_seg_metrics and against each other. Nothing here is a threshold: the tool records times.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import selectivenet_for_semantic_segmentation_binary_amd as S  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT  # noqa: E402


def timed(f, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us per call of f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("patch_report_bench: no GPU visible (timings are taken on the device only)")
    dev = "cuda"
    t_out = MT.logit_threshold("eval", 0.5)
    t_sel = MT.logit_threshold("eval", 0.5)
    print(f"{torch.cuda.get_device_name(0)}; AUC chunk {K.AUC_CHUNK}; {a.iters} calls per timing (forward: "
          f"{max(3, a.iters // 20)}), median of {a.rounds} rounds [min .. max], us")
    ok = True
    for n, side in ((16, 256), (8, 512)):
        hw = side * side
        g = torch.Generator(device="cpu").manual_seed(0)
        out = torch.randn(n, side, side, generator=g).to(dev)
        sel_t = torch.randn(n, side, side, generator=g).to(dev)
        tgt = (torch.rand(n, side, side, generator=g) < 0.4).float().to(dev)
        x = torch.randn(n, 3, side, side, generator=g).to(dev)
        net = S.UNet_B("RGB", selective=True).to(dev).train(False)
        stream = K.stream_ptr()

        def forward():
            with torch.no_grad():
                net(x)

        for name, sel in (("no selection", None), ("selection", sel_t)):
            counts = torch.zeros(6, dtype=torch.int64, device=dev)
            rows = torch.zeros(n, 6, dtype=torch.int64, device=dev)
            auc = torch.zeros(n, 4, dtype=torch.int64, device=dev)
            po, ps, pt = K.ptr(out), K.ptr(sel), K.ptr(tgt)
            pc, pr, pa = K.ptr(counts), K.ptr(rows), K.ptr(auc)
            rep = MT.PatchReport(dev, selective=sel is not None)

            def whole():
                K.call("selunet_seg_metrics", po, ps, pt, n * hw, t_out, t_sel, pc, stream)

            def per_image():
                K.call("selunet_seg_metrics_rows", po, ps, pt, n, hw, t_out, t_sel, pr, stream)

            def patch_auc():
                K.call("selunet_patch_auc", po, ps, pt, n, hw, t_sel, pa, stream)

            def add_batch():
                rep.add_batch(out, tgt, sel)
                rep.reset()

            whole(), per_image(), patch_auc()
            torch.cuda.synchronize()
            c, r, u = counts.cpu().numpy(), rows.cpu().numpy(), auc.cpu().numpy()
            same = bool((r.sum(0) == c).all() and (u[:, 1:].sum(1) == r[:, :4].sum(1)).all()
                        and (u[:, 0] <= 2 * u[:, 1] * u[:, 2]).all() and (u[:, 0] > 0).all())
            ok = ok and same
            fs = {"a": whole, "b": per_image, "c": patch_auc, "d": add_batch, "e": forward}
            for f in fs.values():  # warm-up
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            t = {k: [] for k in fs}
            for _ in range(a.rounds):
                for k, f in fs.items():
                    t[k].append(timed(f, max(3, a.iters // 20) if k == "e" else a.iters))
            med = {k: statistics.median(v) for k, v in t.items()}
            fmt = lambda k: f"{med[k]:10.2f} [{min(t[k]):.2f} .. {max(t[k]):.2f}]"  # noqa: E731
            print(f"{n} x {side} x {side}, {name} (selected {int(c[4])} of {int(c[5])} pixels), counts consistent: {same}")
            print(f"    (a) selunet_seg_metrics, whole batch {fmt('a')}")
            print(f"    (b) selunet_seg_metrics_rows         {fmt('b')}")
            print(f"    (c) selunet_patch_auc                {fmt('c')}")
            print(f"    (d) PatchReport.add_batch            {fmt('d')}")
            print(f"    (e) eval-mode forward, fp32          {fmt('e')}")
            print(f"    (d)/(e) = {med['d'] / med['e']:.4f}", flush=True)
    print("counts consistent in every case:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
