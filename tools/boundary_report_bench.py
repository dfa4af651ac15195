"""Time the boundary report on one eval batch beside the eval-mode forward of the same batch,
and `eval` end to end with and without --boundary_report 1 — measurement tool.

    python tools/boundary_report_bench.py [--iters 20] [--rounds 5] [--patches 256] > profiles/boundary_report.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- \\
        python tools/boundary_report_bench.py --iters 5 --rounds 1 --skip_eval      (per-kernel times)

Part 1, one batch of 128 x 256 x 256 fp32 logits (HIP events around `iters` back-to-back calls after a
warm-up, the variants alternating over `rounds` rounds; median round with the min-max spread):
  (a) selunet_edt_sq of the target, (b) of the output, (c) selunet_boundary_bands, (d) one
  selunet_boundary_rows call, (e) what `metrics.BoundaryReport.add_batch` enqueues for the batch with
  selection, (f) the fp32 eval-mode forward of a selective UNet_B on the batch.
Two kinds of masks: 'regions' — smooth random fields thresholded, regions tens of pixels across with errors
along and away from their contours, every image with both classes; and 'regions, 1 in 4 blank' — the same
with every fourth label and every eighth prediction of one class (the no-contour early exit of the row pass).
Part 2, `eval.evaluate` on synthetic:<patches> at 256 x 256, batch 128, selective, --select_eval 1: wall clock
around the call (it ends in a device-to-host copy), the test set built once and shared, flag off and on
alternating over `rounds` rounds after one warm-up run of each. The off run is the code path without this
feature. Before timing, the distances are checked against a float64 torch brute force on a crop, and the
bands against selunet_seg_metrics. Nothing here is a threshold: the tool records times.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import selectivenet_for_semantic_segmentation_binary_amd as S  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import eval as EV  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT  # noqa: E402


def timed(f, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us per call of f


def fields(n, side, seed, waves, dev):
    """[n][side][side] sums of six sines of up to `waves` periods per side."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(side, dtype=torch.float32), torch.arange(side, dtype=torch.float32),
                            indexing="ij")
    k = torch.rand(n, 6, 2, generator=g) * (waves - 0.3) + 0.3
    p = torch.rand(n, 6, generator=g) * 6.28
    f = torch.zeros(n, side, side)
    for j in range(6):
        f += torch.sin(k[:, j, 0, None, None] * yy * (6.28 / side) + k[:, j, 1, None, None] * xx * (6.28 / side)
                       + p[:, j, None, None])
    return f.to(dev)


def brute_crop(mask):
    """Squared distance to the other class of a small [h][w] bool mask, all pairs in torch."""
    h, w = mask.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=mask.device), torch.arange(w, device=mask.device), indexing="ij")
    ys, xs, m = ys.reshape(-1), xs.reshape(-1), mask.reshape(-1)
    d = (ys[:, None] - ys[None, :]) ** 2 + (xs[:, None] - xs[None, :]) ** 2
    d = torch.where(m[:, None] != m[None, :], d, torch.full_like(d, K.EDT_NONE))
    return d.min(1).values.reshape(h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--patches", type=int, default=256)
    ap.add_argument("--skip_eval", action="store_true", help="part 1 only (a profiler run of the kernels)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("boundary_report_bench: no GPU visible (timings are taken on the device only)")
    dev = "cuda"
    n, side = 128, 256
    hw = side * side
    t_out = MT.logit_threshold("eval", 0.5)
    t_sel = MT.logit_threshold("eval", 0.5)
    print(f"{torch.cuda.get_device_name(0)}; {a.iters} calls per timing (forward: {max(3, a.iters // 5)}), median of "
          f"{a.rounds} rounds [min .. max], us")
    x = torch.randn(n, 3, side, side, generator=torch.Generator(device="cpu").manual_seed(0)).to(dev)
    net = S.UNet_B("RGB", selective=True).to(dev).train(False)
    stream = K.stream_ptr()
    ok = True

    def forward():
        with torch.no_grad():
            net(x)

    for name, blank in (("regions", False), ("regions, 1 in 4 blank", True)):
        tgt = (fields(n, side, 1, 2.0, dev) > 0.2).float()
        out = (fields(n, side, 2, 4.0, dev) + (tgt - 0.5) * 3).contiguous()
        sel = fields(n, side, 3, 4.0, dev)
        if blank:
            tgt[::4] = 0.0
            out[4::8] = -1.0
        rep = MT.BoundaryReport(dev, selective=True)
        d2t = MT.boundary_distance_sq(tgt, 0.5)
        d2p = MT.boundary_distance_sq(out, t_out)
        # checks: a 48 x 48 crop transformed alone against all pairs; the bands against selunet_seg_metrics
        crop = tgt[1:2, 100:148, 60:108].contiguous()
        same = bool((MT.boundary_distance_sq(crop, 0.5)[0] == brute_crop(crop[0] >= 0.5)).all())
        bins = torch.zeros(len(rep.r2) + 2, 6, dtype=torch.int64, device=dev)
        rows = torch.zeros(n, 6, dtype=torch.int64, device=dev)
        counts = torch.zeros(6, dtype=torch.int64, device=dev)
        po, ps, pt, pa, pb = K.ptr(out), K.ptr(sel), K.ptr(tgt), K.ptr(d2t), K.ptr(d2p)

        def edt_target():
            K.call("selunet_edt_sq", pt, 0.5, n, side, side, pa, stream)

        def edt_output():
            K.call("selunet_edt_sq", po, t_out, n, side, side, pb, stream)

        def bands():
            K.call("selunet_boundary_bands", po, ps, pt, pa, n, hw, t_out, t_sel, rep._r2c, len(rep.r2), K.ptr(bins),
                   stream)

        def per_image():
            K.call("selunet_boundary_rows", po, ps, pt, pa, pb, n, hw, t_out, t_sel, rep.tol_sq, K.ptr(rows), stream)

        def add_batch():
            rep.add_batch(out, tgt, sel)
            rep.reset()

        bands(), per_image()
        K.call("selunet_seg_metrics", po, ps, pt, n * hw, t_out, t_sel, K.ptr(counts), stream)
        same = same and bool((bins.sum(0) == counts).all()) and bool((rows[:, 4:].sum() == counts[1] + counts[2]))
        ok = ok and same
        finite = d2t[d2t < K.EDT_NONE]
        print(f"{n} x {side} x {side}, {name}: {int((d2t[:, 0, 0] == K.EDT_NONE).sum())} labels and "
              f"{int((d2p[:, 0, 0] == K.EDT_NONE).sum())} predictions without a contour, label distance mean "
              f"{float(finite.float().sqrt().mean()):.2f} max {float(finite.max()) ** 0.5:.2f} px, "
              f"{int(counts[1] + counts[2])} selected errors, checks pass: {same}")
        fs = {"a": edt_target, "b": edt_output, "c": bands, "d": per_image, "e": add_batch, "f": forward}
        for f in fs.values():  # warm-up
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fs}
        for _ in range(a.rounds):
            for k, f in fs.items():
                t[k].append(timed(f, max(3, a.iters // 5) if k == "f" else a.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        fmt = lambda k: f"{med[k]:10.2f} [{min(t[k]):.2f} .. {max(t[k]):.2f}]"  # noqa: E731
        print(f"    (a) selunet_edt_sq, target            {fmt('a')}")
        print(f"    (b) selunet_edt_sq, output            {fmt('b')}")
        print(f"    (c) selunet_boundary_bands            {fmt('c')}")
        print(f"    (d) selunet_boundary_rows             {fmt('d')}")
        print(f"    (e) BoundaryReport.add_batch          {fmt('e')}")
        print(f"    (f) eval-mode forward, fp32           {fmt('f')}")
        print(f"    ((a)+(b))/(f) = {(med['a'] + med['b']) / med['f']:.4f}   (e)/(f) = {med['e'] / med['f']:.4f}", flush=True)
    print("checks pass in every case:", ok)
    del net, x
    if a.skip_eval:
        return 0 if ok else 1

    # ---- eval end to end
    with tempfile.TemporaryDirectory() as tmp:
        ck = os.path.join(tmp, "checkpoint")
        os.makedirs(ck)
        torch.manual_seed(0)
        torch.save({"net": S.UNet_B("RGB", selective=True).state_dict()}, os.path.join(ck, "model_epoch1.pth"))
        base = ["--data_dir", f"synthetic:{a.patches}", "--patch_size", "256", "--test_fold", "1", "--model_dir", ck,
                "--selective", "1", "--select_eval", "1", "--batch_size", "128", "--save_dir", os.path.join(tmp, "out")]
        args = {"off": EV.parse_arguments(base), "on": EV.parse_arguments(base + ["--boundary_report", "1"])}
        ds = EV.load_test_set(args["off"])
        EV.load_test_set = lambda _args: ds  # the set is built once: the timed window is the pass over it
        sink = open(os.devnull, "w")
        t = {k: [] for k in args}
        for r in range(a.rounds + 1):  # round 0 warms up
            for k, ar in args.items():
                torch.cuda.synchronize()
                stdout, sys.stdout = sys.stdout, sink
                t0 = time.perf_counter()
                try:
                    EV.evaluate(ar)
                finally:
                    sys.stdout = stdout
                if r:
                    t[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"eval, synthetic:{a.patches} at 256 x 256 ({len(ds)} patches), batch 128, selective, --select_eval 1; wall "
              f"clock of evaluate(), ms, median of {a.rounds} alternating runs [min .. max]")
        for k in ("off", "on"):
            print(f"    --boundary_report {k:<3}  {med[k]:10.2f} [{min(t[k]):.2f} .. {max(t[k]):.2f}]")
        print(f"    on - off = {med['on'] - med['off']:.2f} ms ({(med['on'] / med['off'] - 1) * 100:+.2f} %)")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
