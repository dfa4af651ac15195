"""Time fp32 eval-mode forwards of the selective UNet_B on the exact and on the split-fp16 conv path
(`fp32_eval_path`), and the split path's range-word pass (selunet_act_amax) on its own —
measurement tool.

    python tools/eval_forward_bench.py [--iters 20] [--rounds 5] > profiles/eval_split_forward.txt

Per batch shape (16 x 256^2, 8 x 512^2, 128 x 256^2): two modules with the same seed-0 parameters and
running statistics (moved by three training-mode forwards of a small batch), one per path; the logits of
the two paths are compared first. HIP events around `iters` back-to-back forwards (launch-plan replays)
after a warm-up, the two paths alternating over `rounds` rounds; the median round is reported with the
min-max spread. Then selunet_act_amax alone over the 14 CBR layers' [M][C] shapes of that batch (the same
timing), with the bytes it reads (M*C*4) over its time, and the sum of the 14 as a share of the split
forward. Nothing here is a threshold: the tool records times.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import selectivenet_for_semantic_segmentation_binary_amd as S  # noqa: E402
import selectivenet_for_semantic_segmentation_binary_amd.layout as L  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd.engine import fp32_eval_conv_path  # noqa: E402

SHAPES = ((16, 256), (8, 512), (128, 256))


def timed(f, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # ms per call of f


def layer_shapes(n, side):
    """(name, M, C) of the 14 CBR outputs for an n x side x side batch."""
    out = []
    for name, _, co in L.CBR_LAYERS:
        f = 1 << (int(name.split("_")[2]) - 1)
        out.append((name, n * (side // f) * (side // f), co))
    return out


def alternating(fs, iters, rounds):
    for f in fs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fs}
    for _ in range(rounds):
        for k, f in fs.items():
            t[k].append(timed(f, iters))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_forward_bench: no GPU visible (timings are taken on the device only)")
    dev = "cuda"
    print(f"{torch.cuda.get_device_name(0)}; fp32 eval-mode forward of the selective UNet_B, conv paths "
          f"{fp32_eval_conv_path('exact')!r} and {fp32_eval_conv_path('split')!r}; {a.iters} forwards per timing, "
          f"median of {a.rounds} alternating rounds [min .. max]")
    p = L.seeded_params(0, "RGB", True)
    for n, side in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn(n, 3, side, side, generator=g).to(dev)
        nets = {}
        for path in ("exact", "split"):
            net = S.UNet_B("RGB", selective=True, fp32_eval_path=path)
            with torch.no_grad():
                for k, t in net.named_parameters():
                    t.copy_(torch.tensor(p[k]))
            nets[path] = net.to(dev)
        with torch.no_grad():  # running statistics of a small batch of the same distribution
            nets["exact"].train()
            for _ in range(3):
                nets["exact"](x[:2].contiguous())
        nets["split"].load_state_dict(nets["exact"].state_dict())
        for net in nets.values():
            net.train(False)
        outs = {}
        with torch.no_grad():
            for path, net in nets.items():
                outs[path] = [o.clone() for o in net(x)]
        torch.cuda.synchronize()
        rel = max(float((s_ - e_).abs().max() / e_.abs().max()) for s_, e_ in zip(outs["split"], outs["exact"]))
        finite = all(bool(torch.isfinite(o).all()) for o in outs["split"])
        del outs

        def fwd(net):
            def f():
                with torch.no_grad():
                    net(x)
            return f

        iters = max(3, a.iters // 4) if n * side * side > 2 ** 21 else a.iters
        t = alternating({k: fwd(v) for k, v in nets.items()}, iters, a.rounds)
        med = {k: statistics.median(v) for k, v in t.items()}
        fmt = lambda k: f"{med[k]:9.3f} ms [{min(t[k]):.3f} .. {max(t[k]):.3f}]  {med[k] / n:.4f} ms per image"  # noqa: E731
        print(f"{n} x {side} x {side}: logits of the two paths agree to {rel:.2e} of the largest (finite: {finite}); "
              f"{iters} forwards per timing")
        print(f"    exact path {fmt('exact')}")
        print(f"    split path {fmt('split')}")
        spread = max(max(v) - min(v) for v in t.values())
        print(f"    exact / split = {med['exact'] / med['split']:.3f}; difference {med['exact'] - med['split']:.3f} ms, "
              f"largest spread of the alternating rounds {spread:.3f} ms")
        del nets
        torch.cuda.empty_cache()
        # the range-word pass alone
        shapes = layer_shapes(n, side)
        big = max(m * c for _, m, c in shapes)
        y = torch.randn(big, device=dev)
        word = torch.zeros(1, device=dev)
        stream = K.stream_ptr()
        total_us, total_b = 0.0, 0
        print(f"    selunet_act_amax alone, {a.iters} calls per timing:")
        for name, m, c in shapes:
            sc, sh = (torch.randn(c, generator=g).to(dev) for _ in range(2))
            args = (K.ptr(y), m, c, K.ptr(sc), K.ptr(sh), K.ptr(word), stream)
            tt = alternating({"amax": lambda: K.call("selunet_act_amax", *args)}, a.iters, a.rounds)["amax"]
            us = statistics.median(tt) * 1e3
            total_us += us
            total_b += m * c * 4
            print(f"        {name:18s} [{m:9d}][{c:3d}] {m * c * 4 / 1e6:8.1f} MB {us:9.2f} us "
                  f"[{min(tt) * 1e3:.2f} .. {max(tt) * 1e3:.2f}] {m * c * 4 / us / 1e6:6.2f} TB/s")
        print(f"        14 layers: {total_b / 1e6:.1f} MB ({total_b / n / 1e6:.1f} MB per image) {total_us:.1f} us = "
              f"{total_us / 1e3 / med['split']:.3f} of the split forward", flush=True)
        del y
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
