"""Generate tests/golden/patch_perf_cases.npz: the REFERENCE's `get_performance`
(utils/compute_metric.py:93-148) on a dozen flattened patches.

Run once where the reference exists (never on the GPU box):

    python tests/golden/make_patch_perf.py

Per case the inputs (`label` uint8 in {0, 1}, `logit` fp32, `predict` uint8 = logit >= the eval rule's
logit threshold at cut-off 0.5) and the reference's five outputs (accuracy, recall, precision, f1 score,
AUC score; float64, NaN where it returns NaN) are stored. Only data is written.

Two facts about the environment the reference meets here: numpy 2 has no `np.NaN`, which
`get_performance` names, so this process defines it before the call; and sklearn's `roc_auc_score`
rejects non-finite scores (the reference's try/except then returns NaN), so every logit here is finite —
+-inf and NaN logits belong to the numpy comparisons of the GPU tests.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REF, "utils"))

np.NaN = np.NAN = np.nan  # numpy >= 2 dropped the aliases get_performance uses

from compute_metric import get_performance  # noqa: E402  (reference)

from selectivenet_for_semantic_segmentation_binary_amd import metrics as MT  # noqa: E402

F32 = np.float32
T_OUT = F32(MT.logit_threshold("eval", 0.5))


def labels(rng, hw, frac):
    lab = (rng.random(hw) < frac).astype(np.uint8)
    if 0 < frac < 1:  # both classes present whatever the draw
        lab[0], lab[1] = 0, 1
    return lab


def scored(rng, lab, shift=1.0, scale=1.0):
    """Logits that rank label 1 above label 0 by `shift` standard deviations (negative: inverted)."""
    return (rng.normal(0, scale, lab.size) + shift * (lab.astype(np.float64) - 0.5) * 2 * scale).astype(F32)


def cases():
    rng = np.random.Generator(np.random.PCG64(20261019))
    out = {}
    lab = labels(rng, 576, 0.5)
    out["balanced_576"] = (lab, scored(rng, lab))
    lab = labels(rng, 4096, 0.5)
    out["balanced_4096"] = (lab, scored(rng, lab, 0.7))
    lab = labels(rng, 9216, 0.5)
    out["balanced_9216"] = (lab, scored(rng, lab, 1.5, 3.0))
    lab = labels(rng, 4096, 0.05)
    out["pos5_4096"] = (lab, scored(rng, lab))
    lab = labels(rng, 5184, 0.95)
    out["pos95_5184"] = (lab, scored(rng, lab, 0.5))
    lab = labels(rng, 4096, 0.5)
    out["ties_4096"] = (lab, (np.round(scored(rng, lab, 0.6) * 2) / 2).astype(F32))  # quantised to 0.5
    lab = labels(rng, 9216, 0.05)
    out["ties_pos5_9216"] = (lab, (np.round(scored(rng, lab, 0.3) * 2) / 2).astype(F32))
    lab = labels(rng, 1024, 0.5)
    logit = scored(rng, lab, 0.2, 1e-3)
    edge = np.array([0.0, -0.0, 3e38, -3e38, 1e-42, -1e-42], F32)  # signed zeros, near-max, denormals
    at = rng.choice(1024, 8 * len(edge), replace=False)
    logit[at] = np.tile(edge, 8)  # each value on both labels, several times
    out["edge_values_1024"] = (lab, logit)
    lab = labels(rng, 2304, 0.5)
    out["chance_2304"] = (lab, scored(rng, lab, 0.0))
    lab = labels(rng, 1600, 0.95)
    out["inverted_pos95_1600"] = (lab, scored(rng, lab, -0.8))
    lab = labels(rng, 576, 0.5)
    out["inverted_perfect_576"] = (lab, np.where(lab == 1, F32(-1), F32(1)) * (1 + rng.random(576)).astype(F32))
    lab = labels(rng, 576, 1.0)
    out["all_positive_576"] = (lab, scored(rng, lab, 0.0))
    lab = labels(rng, 576, 0.0)
    out["all_negative_576"] = (lab, -np.abs(scored(rng, lab, 0.0)) - F32(1))  # nothing predicted 1 either
    return out


def main():
    arrays, names, perf = {}, [], []
    for name, (lab, logit) in cases().items():
        assert lab.dtype == np.uint8 and logit.dtype == F32 and lab.size % 4 == 0 and 576 <= lab.size <= 9216
        assert np.isfinite(logit).all()
        predict = (logit >= T_OUT).astype(np.uint8)
        got = get_performance(lab, logit, predict)
        names.append(name)
        perf.append([float(v) for v in got])
        arrays[f"label_{name}"], arrays[f"logit_{name}"], arrays[f"predict_{name}"] = lab, logit, predict
        print(f"{name:22s} hw {lab.size:5d} pos {int(lab.sum()):5d}  " + " ".join(f"{v:.6f}" for v in perf[-1]))
    path = os.path.join(HERE, "patch_perf_cases.npz")
    np.savez_compressed(path, names=np.array(names), perf=np.array(perf, np.float64), t_out=T_OUT, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
