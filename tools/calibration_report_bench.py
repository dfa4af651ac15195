"""Time the calibration report: `selunet_calibration_bins` on 16 x 256 x 256 pixels beside
`selunet_seg_metrics_sweep` on the same planes, and `eval` end to end with and without --calibration_report 1
— measurement tool.

    python tools/calibration_report_bench.py [--iters 50] [--rounds 5] [--patches 256] >> profiles/calibration_report.txt

Part 1 (HIP events around `iters` back-to-back calls after a warm-up, the variants alternating over `rounds`
rounds; median round with the min-max spread), 19 eval-rule edges unless said otherwise, with the fine histogram:
  uniform      scores uniform over 102 bins (101 edges): a pixel's bin differs from its lane's last one;
  normal       scores ~ N(0, 3): the spread of an untrained head;
  single bin   every score +inf: one bin, one cell (what a saturated checkpoint gives);
  two ends     scores +-40 in blobs tens of pixels across: the two end bins, as a trained network;
  no fine      the uniform case without the fine histogram;
  event 1      the uniform case with the event "the prediction is right";
  sweep        selunet_seg_metrics_sweep, 11 thresholds, uniform bins (the 12.2 us of DESIGN.md §7b).
Part 2, `eval.evaluate` on synthetic:<patches> at 256 x 256, batch 128, selective, --select_eval 1 (three
views): wall clock around the call, the test set built once and shared, flag off and on alternating over
`rounds` rounds after one warm-up run of each. The off run is the code path without this feature.
Nothing here is a threshold: the tool records times.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--patches", type=int, default=256)
    ap.add_argument("--skip_eval", action="store_true", help="part 1 only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("calibration_report_bench: no GPU visible (timings are taken on the device only)")
    dev = "cuda"
    n, side = 16, 256
    p = n * side * side
    g = torch.Generator(device="cpu").manual_seed(0)
    t_out = MT.logit_threshold("eval", 0.5)
    print(f"{torch.cuda.get_device_name(0)}; {p} pixels, {a.iters} calls per timing, median of {a.rounds} rounds "
          f"[min .. max], us")
    tgt = (torch.rand(p, generator=g) > 0.4).float().to(dev)
    out = torch.randn(p, generator=g).to(dev)
    yy, xx = torch.meshgrid(torch.arange(side, dtype=torch.float32), torch.arange(side, dtype=torch.float32),
                            indexing="ij")
    blobs = torch.stack([torch.sin(yy * (0.05 + 0.01 * i)) + torch.sin(xx * (0.07 + 0.01 * i) + i) for i in range(n)])
    planes = {"uniform": (torch.rand(p, generator=g) * 8.16 - 4.08),
              "normal": torch.randn(p, generator=g) * 3,
              "single bin": torch.full((p,), float("inf")),
              "two ends": torch.where(blobs > 0.3, 40.0, -40.0).reshape(-1)}
    planes = {k: v.contiguous().to(dev) for k, v in planes.items()}
    e19 = torch.tensor(MT.calibration_edges(20)[1], device=dev)
    e101 = torch.linspace(-4, 4, 101, device=dev)
    thr11 = torch.linspace(-4, 4, 11, device=dev)
    bins = torch.zeros(102, 5, dtype=torch.int64, device=dev)
    fine = torch.zeros(K.CALIB_FINE_CELLS, 2, dtype=torch.int64, device=dev)
    misc = torch.zeros(2, dtype=torch.int64, device=dev)
    sweep_bins = torch.zeros(12, 5, dtype=torch.int64, device=dev)
    stream = K.stream_ptr()

    def calib(score, edges, event=0, with_fine=True):
        return lambda: K.call("selunet_calibration_bins", K.ptr(score), K.ptr(out) if event else None, None, K.ptr(tgt),
                              p, event, t_out, t_out, K.ptr(edges), edges.numel(), 1.0, K.ptr(bins),
                              K.ptr(fine) if with_fine else None, K.ptr(misc), stream)

    fs = {"uniform, 101 edges": calib(planes["uniform"], e101), "uniform": calib(planes["uniform"], e19),
          "normal": calib(planes["normal"], e19), "single bin": calib(planes["single bin"], e19),
          "two ends": calib(planes["two ends"], e19),
          "no fine (uniform, 101 edges)": calib(planes["uniform"], e101, with_fine=False),
          "event 1 (uniform, 101 edges)": calib(planes["uniform"], e101, event=1),
          "sweep, 11 thresholds": lambda: K.call("selunet_seg_metrics_sweep", K.ptr(out), K.ptr(planes["uniform"]),
                                                 K.ptr(tgt), p, t_out, K.ptr(thr11), 11, K.ptr(sweep_bins), stream)}
    for f in fs.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fs}
    for _ in range(a.rounds):
        for k, f in fs.items():
            t[k].append(timed(f, a.iters))
    for k in fs:
        print(f"    {k:<32} {statistics.median(t[k]):10.2f} [{min(t[k]):.2f} .. {max(t[k]):.2f}]", flush=True)
    if a.skip_eval:
        return 0

    with tempfile.TemporaryDirectory() as tmp:
        ck = os.path.join(tmp, "checkpoint")
        os.makedirs(ck)
        torch.manual_seed(0)
        torch.save({"net": S.UNet_B("RGB", selective=True).state_dict()}, os.path.join(ck, "model_epoch1.pth"))
        base = ["--data_dir", f"synthetic:{a.patches}", "--patch_size", "256", "--test_fold", "1", "--model_dir", ck,
                "--selective", "1", "--select_eval", "1", "--batch_size", "128", "--save_dir", os.path.join(tmp, "out")]
        args = {"off": EV.parse_arguments(base), "on": EV.parse_arguments(base + ["--calibration_report", "1"])}
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
            print(f"    --calibration_report {k:<3}  {med[k]:10.2f} [{min(t[k]):.2f} .. {max(t[k]):.2f}]")
        print(f"    on - off = {med['on'] - med['off']:.2f} ms ({(med['on'] / med['off'] - 1) * 100:+.2f} %)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
