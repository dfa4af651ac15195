"""Time the augmenting batch preparation beside today's — measurement tool.

    python tools/augment_prep_bench.py [--iters 500] [--rounds 9] [--parent_lib PATH] [--step_ms MS] \
        >> profiles/augment_prep.txt

One process, n = 128 patches of 256 x 256, 'RGB', the same uint8 batch for every variant:
  (a) selunet_prep_batch_mode with the two flips — the call training makes without augmentation. With
      --parent_lib it is taken from that libselunet.so (a build of the commit before the augmentation) loaded
      beside this tree's; without, from this tree's library, whose prep_batch_kernel is the same source;
  (b) selunet_prep_batch_aug with the same flips and nothing else (geom in 0..3, no glass, no table);
  (c) selunet_prep_batch_aug with everything on: all eight orientations (half the images transposed), every
      second image a glass quadrant, a colour table per image;
  (c') the same without the transposes (geom & 3), to price the strided source reads of (c) alone.
HIP events around `iters` back-to-back calls after a warm-up of every variant, the variants alternating over
`rounds` rounds; per variant the median round with its min .. max, and for (a) that spread is the run-to-run
spread the other rows are read against. --step_ms: the training step time of the same machine (bench.py's
ms_per_step), to state (c) as a share of a step. The tool records; it asserts nothing.
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import data as D  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent_lib", default=None, help="libselunet.so of the commit before the augmentation, for (a)")
    ap.add_argument("--step_ms", type=float, default=None, help="bench.py's ms_per_step on this machine")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_prep_bench: no GPU visible (timings are taken on the device only)")
    dev = "cuda"
    n, side = 128, 256
    ds = D.synthetic_patchset(n, side, seed=0)
    rng = np.random.Generator(np.random.PCG64(0))
    img, lab = torch.from_numpy(np.asarray(ds.images)).to(dev), torch.from_numpy(np.asarray(ds.labels)).to(dev)
    geom = torch.from_numpy((np.arange(n) % 8).astype(np.uint8)).to(dev)
    flips = geom & 3
    glass = torch.from_numpy((np.arange(n) % 2 * (np.arange(n) // 2 % 4 + 1)).astype(np.uint8)).to(dev)
    keys = torch.from_numpy(rng.integers(0, 2 ** 32, n, dtype=np.uint32).view(np.int32)).to(dev)
    lut = torch.from_numpy(D.color_lut(rng.uniform(0.8, 1.2, (n, 3)), rng.uniform(-0.2, 0.2, (n, 3)))).to(dev)
    table = torch.from_numpy(D.glass_table().copy()).to(dev)
    x = torch.empty(n, 3, side, side, device=dev)
    t = torch.empty(n, side, side, device=dev)
    stream = K.stream_ptr()

    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.selunet_prep_batch_mode.restype, parent.selunet_prep_batch_mode.argtypes = \
            K.SIGNATURES["selunet_prep_batch_mode"]
        assert not hasattr(parent, "selunet_prep_batch_aug"), "--parent_lib: a library from before the augmentation"

        def mode():
            rc = parent.selunet_prep_batch_mode(K.ptr(img), K.ptr(lab), K.ptr(flips), n, side, side, 0, K.ptr(x),
                                                K.ptr(t), stream)
            assert rc == 0
        a_name = "(a) prep_batch_mode, flips (the parent's library)"
    else:
        def mode():
            K.call("selunet_prep_batch_mode", K.ptr(img), K.ptr(lab), K.ptr(flips), n, side, side, 0, K.ptr(x), K.ptr(t),
                   stream)
        a_name = "(a) prep_batch_mode, flips (this tree's library)"

    def aug(g, gl, ky, lu, tb, tr):
        return lambda: K.call("selunet_prep_batch_aug", K.ptr(img), K.ptr(lab), K.ptr(g), K.ptr(gl), K.ptr(ky), K.ptr(lu),
                              K.ptr(tb), tr, n, side, side, 0, K.ptr(x), K.ptr(t), stream)

    fs = {a_name: mode,
          "(b) prep_batch_aug, the same flips only": aug(flips, None, None, None, None, 0),
          "(c) prep_batch_aug, d4 + glass + colour": aug(geom, glass, keys, lut, table, 1),
          "(c') the same without the transposes": aug(flips, glass, keys, lut, table, 0)}
    # (a) and (b) compute the same thing
    mode()
    xa, ta = x.clone(), t.clone()
    fs["(b) prep_batch_aug, the same flips only"]()
    assert torch.equal(xa.view(torch.int32), x.view(torch.int32)) and torch.equal(ta, t)
    for f in fs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    tm = {k: [] for k in fs}
    for _ in range(a.rounds):
        for k, f in fs.items():
            tm[k].append(timed(f, a.iters))
    px = n * side * side
    print(f"{torch.cuda.get_device_name(0)}; {n} x {side} x {side} 'RGB' ({px * 20 / 1e6:.0f} MB read + written per "
          f"call at 20 B per pixel), {a.iters} calls per timing, median of {a.rounds} alternating rounds [min .. max], us")
    med = {k: statistics.median(v) for k, v in tm.items()}
    for k in fs:
        print(f"    {k:<52} {med[k]:9.2f} [{min(tm[k]):.2f} .. {max(tm[k]):.2f}]   {px * 20 / med[k] / 1e6:.2f} TB/s")
    ka, kb, kc = list(fs)[:3]
    print(f"    run-to-run spread of (a): {max(tm[ka]) - min(tm[ka]):.2f} us "
          f"({(max(tm[ka]) / min(tm[ka]) - 1) * 100:.2f} % of its fastest round)")
    inside = min(tm[ka]) <= med[kb] <= max(tm[ka])
    print(f"    (b) median - (a) median = {med[kb] - med[ka]:+.2f} us; (b)'s median is "
          f"{'inside' if inside else 'OUTSIDE'} (a)'s min .. max")
    if a.step_ms:
        print(f"    training step on this machine (bench.py ms_per_step): {a.step_ms:.2f} ms; (c) = "
              f"{med[kc] / (a.step_ms * 1e3) * 100:.3f} % of it, (c) - (a) = "
              f"{(med[kc] - med[ka]) / (a.step_ms * 1e3) * 100:.3f} % (bar: (c) under 1 %)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
