"""Times the four stain-normalisation passes on a synthetic H&E image, with `tissue_plane` in the
same run as the yardstick of a one-pass byte kernel, then the same calls under several grid caps.

    python tools/stain_norm_bench.py [--size 4096] [--out profiles/stain_norm.txt]

HIP events around each of 20 repetitions after 3 warm-ups; median (min .. max)."""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import predict as PR  # noqa: E402
from selectivenet_for_semantic_segmentation_binary_amd import stain as ST  # noqa: E402
from tests import _stain_ref as R  # noqa: E402

WARM, REPS = 3, 20
GRIDS = (-1, 256, 512, 1024, 2048, 4096, 8192, 16384)


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(REPS + 1)]
    ev[0].record()
    for i in range(REPS):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(REPS))
    return ts[len(ts) // 2], ts[0], ts[-1]


def wall(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "stain_norm.txt"))
    args = ap.parse_args()
    H = W = args.size
    img = torch.from_numpy(R.synthetic_he(H, W, seed=0)).cuda()
    dv, bq = ST._DEVICE, ST.beta_q_of(ST.BETA)
    fit = ST.fit(img)
    acc = dv.zeros(10, img)
    dv.moments(img, bq, acc)
    B = ST.basis_q(*ST.basis_of(dv.read(acc)))
    P_q = ST.pinv_q(fit.HE)[1]
    T = ST.transform(fit, ST.MACENKO_TARGET)
    T_q = ST.transform_q(T)
    a10, aA, aC = dv.zeros(10, img), dv.zeros(ST.K_BINS + 1, img), dv.zeros(2 * ST.C_BINS, img)
    out = torch.empty_like(img)
    od, ex, _ = dv._tables(img.device)

    def apply_into():
        K.call("selunet_stain_apply", K.ptr(img), H, W, K.ptr(od), T_q.ctypes.data, K.ptr(ex), ex.numel(), K.ptr(out),
               K.stream_ptr())

    px = H * W
    rows = [("selunet_stain_moments", lambda: dv.moments(img, bq, a10), 3 * px),
            ("selunet_stain_angle_hist", lambda: dv.angle_hist(img, bq, B, aA), 3 * px),
            ("selunet_stain_conc_hist", lambda: dv.conc_hist(img, bq, P_q, aC), 3 * px),
            ("selunet_stain_apply", apply_into, 6 * px),
            ("selunet_tissue_plane", lambda: PR.tissue_plane(img), 4 * px)]
    lines = [f"Macenko stain normalisation on one MI355X, {H} x {W} synthetic H&E image (tests/_stain_ref.synthetic_he, "
             f"seed 0): {fit.n_stained} stained pixels, {fit.skipped} skipped.",
             f"HIP events around each of {REPS} repetitions after {WARM} warm-ups, one process, one run; median (min .. max).",
             f"library build {K.load().selunet_build_id().decode()}", "",
             f"{'call':28s} {'ms':>8s} {'min':>8s} {'max':>8s} {'MB moved':>9s} {'GB/s':>8s}"]
    res = {}
    for name, fn, nbytes in rows:
        med, lo, hi = timed(fn)
        res[name] = (med, nbytes)
        lines.append(f"{name:28s} {med:8.4f} {lo:8.4f} {hi:8.4f} {nbytes / 1e6:9.1f} {nbytes / med / 1e6:8.1f}")
    base = res["selunet_tissue_plane"][0] / res["selunet_tissue_plane"][1]
    lines.append("")
    for name, (med, nbytes) in res.items():
        lines.append(f"{name:28s} time per byte moved = {med / nbytes / base:5.2f} x tissue_plane's")
    lines.append("")
    for name, fn in (("stain.fit (3 passes, 3 reads, host steps)", lambda: ST.fit(img)),
                     ("stain.apply (1 pass, new image)", lambda: ST.apply(img, T)),
                     ("stain.normalize", lambda: ST.normalize(img))):
        med, lo, hi = wall(fn)
        lines.append(f"{name:44s} wall {med:8.3f} ms ({lo:.3f} .. {hi:.3f})")
    lines += ["", f"non-zero bins: angle {int((dv.read(aA)[:ST.K_BINS] > 0).sum())} of {ST.K_BINS}, concentration "
                  f"{(dv.read(aC).reshape(2, -1) > 0).sum(axis=1).tolist()} of {ST.C_BINS}", "",
              "The same calls under a capped grid (the option IO_GRID; -1: the launchers' own caps, 2048 workgroups of 256 "
              "threads for the four", "stain calls, 8192 for tissue_plane), median ms:", "",
              "grid cap  " + "  ".join(f"{n[len('selunet_'):]:>16s}" for n, _, _ in rows)]
    for grid in GRIDS:
        prev = K.set_option("IO_GRID", grid)
        try:
            lines.append(f"{grid:8d}  " + "  ".join(f"{timed(fn)[0]:16.4f}" for _, fn, _ in rows))
        finally:
            K.set_option("IO_GRID", prev)
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
