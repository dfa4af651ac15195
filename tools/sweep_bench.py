"""Time the one-pass risk-coverage sweep (selunet_seg_metrics_sweep) against what it replaces, a loop of
one selunet_seg_metrics call per cut-off, on one eval batch (16 x 256 x 256 fp32 logits) — measurement
tool.

    python tools/sweep_bench.py [--batch 16] [--iters 2000] [--rounds 5] > profiles/seg_metrics_sweep.txt

Per k (11 and 101 thresholds) and per selection-score distribution (uniform over the k+1 bins; every
pixel in one bin, the case of a trained network whose scores cluster):
  (a) one selunet_seg_metrics call, (b) k such calls, (c) one selunet_seg_metrics_sweep call.
HIP events around `iters` back-to-back calls after a warm-up, the three variants alternating over
`rounds` rounds; the median round is reported with the min-max spread. Before timing, the sweep's
suffix-summed bins are compared with the k calls' counts (they must be equal).
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sweep_bench: no GPU visible (timings are taken on the device only)")
    dev = "cuda"
    p = a.batch * 256 * 256
    g = torch.Generator(device="cpu").manual_seed(0)
    out = torch.randn(p, generator=g).to(dev)
    tgt = (torch.rand(p, generator=g) > 0.4).float().to(dev)
    t_out = MT.logit_threshold("eval", 0.5)
    print(f"{torch.cuda.get_device_name(0)}; batch {a.batch} x 256 x 256 = {p} pixels, {12 * p / 1e6:.1f} MB read per "
          f"pass; {a.iters} calls per timing, median of {a.rounds} rounds [min .. max], us")
    ok = True
    for k in (11, 101):
        cuts, thr = MT.sweep_thresholds(np.linspace(0, 1, k + 2)[1:-1])  # k finite, distinct thresholds
        thr_d = torch.tensor(thr, device=dev)
        edges = np.concatenate([[thr[0] - 1], thr, [thr[-1] + 1]]).astype(np.float64)
        which = torch.randint(0, k + 1, (p,), generator=g).numpy()
        uniform = edges[which] + (edges[which + 1] - edges[which]) * torch.rand(p, generator=g, dtype=torch.float64).numpy()
        one_bin = np.full(p, 0.5 * (edges[k // 2] + edges[k // 2 + 1]))
        for dist, sel_h in (("uniform over the bins", uniform), ("all in one bin", one_bin)):
            sel = torch.tensor(sel_h.astype(np.float32), device=dev)
            counts = torch.zeros(k, 6, dtype=torch.int64, device=dev)
            bins = torch.zeros(k + 1, 5, dtype=torch.int64, device=dev)
            stream = K.stream_ptr()
            # pointers and thresholds formed once: the timed loops are the C-ABI calls alone
            po, ps, pt, pth, pb = (K.ptr(x) for x in (out, sel, tgt, thr_d, bins))
            pc = [counts.data_ptr() + 6 * 8 * j for j in range(k)]
            tj = [float(v) for v in thr]

            def single(j=k // 2):
                K.call("selunet_seg_metrics", po, ps, pt, p, t_out, tj[j], pc[j], stream)

            def loop():
                for j in range(k):
                    single(j)

            def sweep():
                K.call("selunet_seg_metrics_sweep", po, ps, pt, p, t_out, pth, k, pb, stream)

            loop()
            sweep()
            torch.cuda.synchronize()
            b = bins.cpu().numpy()
            rows = np.cumsum(b[::-1], axis=0)[::-1][1:]
            same = np.array_equal(rows, counts.cpu().numpy()[:, :5]) and int(b[:, 4].sum()) == p
            filled = int(np.count_nonzero(b[:, 4]))
            for f in (single, loop, sweep):  # warm-up
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            t = {"a": [], "b": [], "c": []}
            for _ in range(a.rounds):
                t["a"].append(timed(single, a.iters))
                t["b"].append(timed(loop, max(3, a.iters // k)))
                t["c"].append(timed(sweep, a.iters))
            med = {n: statistics.median(v) for n, v in t.items()}
            fmt = lambda n: f"{med[n]:9.2f} [{min(t[n]):.2f} .. {max(t[n]):.2f}]"  # noqa: E731
            print(f"k={k:3d}, {dist} ({filled} of {k + 1} bins filled), counts equal: {same}")
            print(f"    (a) one seg_metrics call      {fmt('a')}")
            print(f"    (b) {k:3d} seg_metrics calls      {fmt('b')}")
            print(f"    (c) one seg_metrics_sweep call{fmt('c')}   {12 * p / med['c'] / 1e6:.2f} TB/s of inputs")
            print(f"    (c)/(a) = {med['c'] / med['a']:.2f}   (c)/(b) = {med['c'] / med['b']:.3f}   "
                  f"(c) < (b): {med['c'] < med['b']}", flush=True)
            ok = ok and same and med["c"] < med["b"]
    print("sweep pays for itself in every case:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
