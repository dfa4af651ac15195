"""Evaluation CLI mirroring the reference's eval.py on the MI355X path (forward-only).

    python -m selectivenet_for_semantic_segmentation_binary_amd.eval --data_dir /data --test_fold 1 \\
        --model_dir /model/1-fold/checkpoint --model_arch UNet_B --selective 1 --select_eval 1

Same flags and defaults as eval.py:17-58 (argparse `type=bool` quirk included), same model loading
(every *.pth in --model_dir, sorted, `module.` prefixes stripped, eval.py:116-154), same
prediction rule — fp32 numpy sigmoid then `> --cut_off` (eval.py:171,175,229-231), selection
`> --s_cut_off` when --select_eval (eval.py:236-246) — and the same Evaluator report
(eval.py:258-279). The forward runs in eval mode with the running BatchNorm statistics on the GPU;
masks and the confusion matrix are computed on the device (`metrics.SegMetrics`, thresholds exact
by construction) and read once at the end.

Ensembles (several checkpoints, selective off, eval.py:185-199) average the per-model outputs on
the GPU in the reference's order; with --ens_scale sigmoid the GPU's exp differs from numpy's by
an ulp on some pixels (parity unpinned for that mode); None / clip / minmax are exact.
Risk-coverage sweep (MI355X path only): --s_cut_off_sweep F [F ...] or --s_cut_off_steps N evaluates
every selection cut-off of the list in the same single pass (`metrics.SelectiveSweep`, counts equal to
a run with that --s_cut_off alone) and writes risk_coverage.json / .csv next to performance.json;
--target_coverage C adds the largest cut-off of the list whose coverage is still >= C.
Per-patch report (MI355X path only): --patch_report 1 writes one row per test patch from the same pass
(`metrics.PatchReport`: confusion matrix, the reference's unused `get_performance` metrics of
utils/compute_metric.py:93-148 with an exact ROC AUC of the logit; with --select_eval also over the
selected pixels) to patch_performance.csv and a summary to patch_performance.json.
Boundary report (MI355X path only): --boundary_report 1 adds the distance view from the same pass
(`metrics.BoundaryReport`): an exact on-device Euclidean distance transform of the label and
prediction masks, the Evaluator's counts, coverage and risk by band of distance to the label contour
(--boundary_bands R [R ...], default 1 2 4 8 16) in boundary_bands.json / .csv, and per patch the Hausdorff
distance and the scores that forgive errors within --boundary_tolerance T (default 2) pixels of the other mask
in patch_boundary.csv, with a summary in patch_boundary.json. Over the selected pixels with --select_eval.
Calibration report (MI355X path only): --calibration_report 1 asks whether the scores can be read as probabilities,
from the same pass (`metrics.CalibrationReport`): per view (tumor; tumor_selected with --select_eval;
selection — the selection score against "the prediction is right" — with --selective) the reliability table over
--calibration_bins K (default 20, even, 2..256) equal-width probability bins, ECE, top-label ECE, MCE, Brier score
and NLL, and the temperature that minimises the NLL, in calibration.json and calibration_bins.csv;
--calibration_temperature T (default 1) reports the tumor views of sigmoid(logit / T), so a fitted T can be checked
by a second run. The outputs must be logits: --single_scale sigmoid, and --ens_scale None for an ensemble.
fp32 conv path (MI355X path only): --fp32_path split runs the fp32 forward on the training forward's
split-fp16 kernels (`UNet_B(fp32_eval_path="split")`); the default, exact, keeps the exact
fp32 kernels. Not with --compute_dtype bf16.
A single process evaluates on the first id of --local_rank (the reference's DataParallel split
of an eval batch changes nothing in eval mode).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np


def parse_arguments(argv=None):
    """eval.py:17-58."""
    parser = argparse.ArgumentParser()
    parser.add_argument('--data_dir', type=str, default='./data')
    parser.add_argument('--test_fold', type=int, default=1, help='which fold in 5-fold cv')
    parser.add_argument('--input_type', type=str, default='RGB')
    parser.add_argument('--patch_mag', type=int, default=200)
    parser.add_argument('--patch_size', type=int, default=256)
    parser.add_argument('--n_cls', type=int, default=2)
    parser.add_argument('--batch_size', type=int, default=16)
    parser.add_argument('--num_workers', type=int, default=16, help='Dataloader num_workers')
    parser.add_argument('--model_dir', type=str, default='*/model', help='network ckpt (.pth) directory')
    parser.add_argument('--model_arch', type=str, nargs='+', default=['UNet_B'], choices=['UNet_B'])
    parser.add_argument('--selective', type=bool, default=False, help='Is the network based on SelectiveNet?')
    parser.add_argument('--select_eval', type=bool, default=False, help='calculate metrics with/without selection')
    parser.add_argument('--output_dim', type=str, default='NHW', choices=['NCHW', 'NHW'])
    parser.add_argument('--single_scale', type=str, default='sigmoid', choices=['None', 'clip', 'sigmoid', 'minmax'])
    parser.add_argument('--ens_scale', type=str, default='None', choices=['None', 'clip', 'sigmoid', 'minmax'])
    parser.add_argument('--cut_off', type=float, default=0.5, help='prob > cut_off -> pred: 1')
    parser.add_argument('--s_cut_off', type=float, default=0.5, help='selection > cut_off -> select: 1')
    parser.add_argument('--local_rank', type=int, nargs='+', default=[0], help='local gpu ids')
    parser.add_argument('--info_print', type=bool, default=False)
    parser.add_argument('--save_dir', type=str, default='./output', help='saving results')
    # ---- MI355X path options
    parser.add_argument('--compute_dtype', type=str, default='fp32', choices=['fp32', 'bf16'])
    sweep = parser.add_mutually_exclusive_group()
    sweep.add_argument('--s_cut_off_sweep', type=float, nargs='+', default=None,
                       help='selection cut-offs of a one-pass risk-coverage sweep')
    sweep.add_argument('--s_cut_off_steps', type=int, default=None,
                       help='N: sweep the N+1 cut-offs linspace(0, 1, N+1) (N <= 255)')
    parser.add_argument('--target_coverage', type=float, default=None,
                        help='with a sweep: report the largest cut-off whose coverage is >= this')
    parser.add_argument('--patch_report', type=bool, default=False,
                        help='write one row per test patch (patch_performance.csv / .json)')
    parser.add_argument('--fp32_path', type=str, default='exact', choices=['exact', 'split'],
                        help='conv kernels of the fp32 forward: exact fp32, or the split-fp16 kernels of training')
    parser.add_argument('--boundary_report', type=bool, default=False,
                        help='errors and rejections by distance to the label contour, Hausdorff distance per patch '
                             '(boundary_bands.json / .csv, patch_boundary.csv / .json)')
    parser.add_argument('--boundary_bands', type=float, nargs='+', default=[1, 2, 4, 8, 16],
                        help='outer radii (pixels) of the distance bands, strictly increasing from >= 1')
    parser.add_argument('--boundary_tolerance', type=float, default=2,
                        help='errors within this distance (pixels) of the other mask count as correct in the '
                             'tolerant scores')
    parser.add_argument('--calibration_report', type=bool, default=False,
                        help='reliability table, ECE, Brier score, NLL and a temperature fit of the scores '
                             '(calibration.json, calibration_bins.csv)')
    parser.add_argument('--calibration_bins', type=int, default=20,
                        help='equal-width probability bins of the reliability table: even, 2..256')
    parser.add_argument('--calibration_temperature', type=float, default=1.0,
                        help='report the tumor views of sigmoid(logit / T) (the fitted T of an earlier run)')
    args = parser.parse_args(argv)
    if args.calibration_report:
        if not 2 <= args.calibration_bins <= 256 or args.calibration_bins % 2:
            parser.error('--calibration_bins: an even number of bins in [2, 256]')
        if not 0 < args.calibration_temperature < float('inf'):
            parser.error('--calibration_temperature: a finite temperature > 0')
    else:
        # off: as the boundary flags below
        for name in ('calibration_report', 'calibration_bins', 'calibration_temperature'):
            delattr(args, name)
    if args.boundary_report:
        from . import metrics as MT
        try:
            MT.band_edges_sq(args.boundary_bands)
        except ValueError as e:
            parser.error(f'--boundary_bands: {e}')
        if not 0 <= args.boundary_tolerance < 4096 * 2 ** 0.5:
            parser.error('--boundary_tolerance: a distance in pixels, >= 0 and below the diagonal of 4096 x 4096')
    else:
        # off: the namespace, and with it the printed args= line, is what it is without the three flags
        for name in ('boundary_report', 'boundary_bands', 'boundary_tolerance'):
            delattr(args, name)
    if args.fp32_path == 'split' and args.compute_dtype == 'bf16':
        parser.error('--fp32_path split is an fp32 path: not with --compute_dtype bf16')
    if args.s_cut_off_steps is not None and not 1 <= args.s_cut_off_steps <= 255:
        parser.error('--s_cut_off_steps: N must be in [1, 255]')
    if args.target_coverage is not None and sweep_cut_offs(args) is None:
        parser.error('--target_coverage needs --s_cut_off_sweep or --s_cut_off_steps')
    return args


def sweep_cut_offs(args):
    """The cut-offs of the requested risk-coverage sweep, or None without one."""
    if args.s_cut_off_sweep is not None:
        return [float(c) for c in args.s_cut_off_sweep]
    if args.s_cut_off_steps is not None:
        return np.linspace(0, 1, args.s_cut_off_steps + 1).tolist()
    return None


def load_test_set(args):
    from . import data as D

    if args.data_dir.startswith("synthetic"):
        return D.PatchSet(*D.load_test_set_for_tests(args.data_dir, args.patch_size, args.test_fold))
    test_list = D.construct_test(args.data_dir, test_fold=args.test_fold)
    return D.decode_patch_list(args.data_dir, test_list, args.patch_mag, args.patch_size)


def evaluate(args):
    import torch

    import selectivenet_for_semantic_segmentation_binary_amd as S
    from . import data as D
    from . import metrics as MT
    from . import net_utils

    if args.input_type not in ('RGB', 'GH', 'H_RGB'):
        raise ValueError(f"input_type {args.input_type!r}: 'RGB', 'GH' or 'H_RGB' (utils/data_utils.py:223-226)")
    cut_offs = sweep_cut_offs(args)
    if cut_offs is not None and not args.selective:
        raise ValueError("a selection cut-off sweep needs a selective network (--selective 1)")
    if getattr(args, "calibration_report", False):  # the report reads the outputs as logits
        if args.single_scale != 'sigmoid':
            raise ValueError(f"--calibration_report needs --single_scale sigmoid (got {args.single_scale!r}): "
                             "the outputs are read as logits")
        if args.ens_scale != 'None' and len([c for c in os.listdir(args.model_dir) if 'pth' in c]) > 1:
            raise ValueError(f"--calibration_report with an ensemble needs --ens_scale None (got {args.ens_scale!r}): "
                             "a mean of logits is a logit, a mean of scaled outputs is not")
    device = torch.device("cuda", args.local_rank[0])
    torch.cuda.set_device(device)
    dt = torch.bfloat16 if args.compute_dtype == 'bf16' else torch.float32
    model_list = sorted(c for c in os.listdir(args.model_dir) if 'pth' in c)
    if not model_list:
        raise FileNotFoundError(f"no .pth checkpoints in {args.model_dir}")
    arch = args.model_arch * len(model_list) if len(args.model_arch) == 1 else args.model_arch
    nets = []
    for name, a in zip(model_list, arch):
        if args.info_print:
            print(f'    {os.path.join(args.model_dir, name)} - {a} / SelectiveNet: {args.selective}')
        net = S.UNet_B(args.input_type, selective=args.selective, compute_dtype=dt,
                       fp32_eval_path=getattr(args, "fp32_path", "exact"))
        net_utils.net_test_load(os.path.join(args.model_dir, name), net)
        nets.append(net.to(device).train(False))
    if len(nets) > 1 and args.selective:
        raise NotImplementedError("ensembles of selective networks are not supported (eval.py:185, '선택 불가')")

    ds = load_test_set(args)
    loader = D.BatchLoader(ds, args.batch_size, shuffle=False, random_flip=False, device=device,
                           input_type=args.input_type)
    ev = MT.SegMetrics(device, selective=bool(args.select_eval), rule="eval", cut_off=args.cut_off,
                       s_cut_off=args.s_cut_off, output_scale=args.single_scale)
    sweep = None if cut_offs is None else MT.SelectiveSweep(device, cut_offs, rule="eval", cut_off=args.cut_off,
                                                            output_scale=args.single_scale)
    report = None
    if getattr(args, "patch_report", False):
        report = MT.PatchReport(device, selective=bool(args.select_eval), rule="eval", cut_off=args.cut_off,
                                s_cut_off=args.s_cut_off, output_scale=args.single_scale)
    boundary = None
    if getattr(args, "boundary_report", False):
        boundary = MT.BoundaryReport(device, selective=bool(args.select_eval), radii=args.boundary_bands,
                                     tolerance=args.boundary_tolerance, rule="eval", cut_off=args.cut_off,
                                     s_cut_off=args.s_cut_off, output_scale=args.single_scale)
    calibration = None
    if getattr(args, "calibration_report", False):
        calibration = MT.CalibrationReport(device, selective=bool(args.selective), select_eval=bool(args.select_eval),
                                           bins=args.calibration_bins, temperature=args.calibration_temperature,
                                           cut_off=args.cut_off, s_cut_off=args.s_cut_off)
    seen = 0  # patches fed so far: the loader walks the set in order
    print("Model Prediction...")
    with torch.no_grad():
        for x, target in loader:
            selection = None
            if len(nets) == 1:
                if args.selective:
                    output, selection, _ = nets[0](x)
                else:
                    output = nets[0](x)
            else:
                acc = None
                for net in nets:  # eval.py:185-199: mean of the scaled outputs, in model order
                    o = net(x)
                    if args.ens_scale == 'clip':
                        o = o.clamp(0, 1)
                    elif args.ens_scale == 'minmax':
                        o = (o - o.min()) / (o.max() - o.min())
                    elif args.ens_scale == 'sigmoid':
                        o = 1 / (1 + torch.exp(-o))
                    acc = o.clone() if acc is None else acc.add_(o)
                output = acc.div_(float(len(nets)))
            if args.select_eval and selection is None:
                raise ValueError("--select_eval needs a selective network (--selective 1)")
            output = output.contiguous()
            selection = None if selection is None else selection.contiguous()
            ev.add_batch(output, target, selection)
            if sweep is not None:
                sweep.add_batch(output, target, selection)
            n = output.shape[0]
            ids = None if ds.ids is None else list(ds.ids[seen:seen + n])
            seen += n
            if report is not None:
                report.add_batch(output, target, selection, ids=ids)
            if boundary is not None:
                boundary.add_batch(output, target, selection, ids=ids)
            if calibration is not None:
                calibration.add_batch(output, target, selection)
    cm =ev.confusion_matrix()
    selected, total = ev.selected_total()
    prec, rec = MT.precision(cm), MT.recall(cm)
    with np.errstate(invalid="ignore", divide="ignore"):
        f1 = 2 * (prec * rec) / (prec + rec)
        acc_class = np.nanmean(np.diag(cm) / cm.sum(axis=1))
        iou_class = np.diag(cm) / (cm.sum(1) + cm.sum(0) - np.diag(cm))
    res = {"confusion_matrix": cm.tolist(), "Acc": float(MT.pixel_accuracy(cm)), "Acc_class": float(acc_class),
           "Prec": prec.tolist(), "Recall": rec.tolist(), "F1_Score": f1.tolist(), "mIoU": float(MT.mean_iou(cm)),
           "IoU_class": iou_class.tolist()}
    print(cm)
    if args.select_eval:
        res["rejection_ratio"] = (total - selected) / max(total, 1)
        print(f'    rejection ratio: {round(res["rejection_ratio"], 3)}')
    print(f'    Acc:{res["Acc"]}')
    print(f'    Acc_class:{res["Acc_class"]}')
    print(f'    Prec:{prec}, Recall:{rec}, F1_Score:{f1}')
    print(f'    mIoU:{res["mIoU"]}')
    print(f'    IoU_class:{iou_class}')
    os.makedirs(args.save_dir, exist_ok=True)
    _write_json(args.save_dir, "performance.json", res)
    if sweep is not None:
        res = dict(res, risk_coverage=report_sweep(sweep.curve(), args.target_coverage, args.save_dir))
    if report is not None:
        res = dict(res, patch_report=report_patches(report.rows(), args.save_dir))
    if boundary is not None:
        res = dict(res, boundary_report=report_boundary(boundary.bands(), boundary.rows(), boundary.radii,
                                                        boundary.tolerance, args.save_dir))
    if calibration is not None:
        res = dict(res, calibration_report=report_calibration(calibration.report(), args.save_dir))
    return res


def _cell(v):
    """A CSV cell: integers as integers, floats by repr."""
    return repr(v) if isinstance(v, float) else str(v)


def _write_csv(save_dir, name, columns, rows):
    """The header line, then one line per row (a sequence of cell values)."""
    with open(os.path.join(save_dir, name), "w") as fh:
        fh.write(",".join(columns) + "\n")
        for r in rows:
            fh.write(",".join(_cell(v) for v in r) + "\n")


def _write_json(save_dir, name, doc):
    with open(os.path.join(save_dir, name), "w") as fh:
        json.dump(doc, fh, indent=1)


def report_calibration(doc, save_dir):
    """Print one line per view of `metrics.CalibrationReport.report()` and write calibration.json (the whole
    document) and calibration_bins.csv (one row per view and reliability bin)."""
    from . import metrics as MT

    print(f'    calibration report ({doc["bins"]} bins):')
    print('    ' + f'{"view":>14} {"pixels":>12} ' + ' '.join(
        f'{c:>10}' for c in ("ECE", "top ECE", "MCE", "Brier", "NLL", "fitted T", "NLL at T")))
    for name, v in doc["views"].items():
        s, f = v["summary"], v["fit"]
        print('    ' + f'{name:>14} {s["pixels"]:12d} ' + ' '.join(
            f'{x:10.6f}' for x in (s["ece"], s["top_label_ece"], s["mce"], s["brier"], s["nll"], f["temperature"],
                                   f["nll_fitted"])))
    os.makedirs(save_dir, exist_ok=True)
    _write_json(save_dir, "calibration.json", doc)
    _write_csv(save_dir, "calibration_bins.csv", ("view",) + MT.CALIBRATION_BIN_COLUMNS,
               ([name] + [r[c] for c in MT.CALIBRATION_BIN_COLUMNS] for name, v in doc["views"].items() for r in v["table"]))
    return doc


def report_boundary(bands, rows, radii, tolerance, save_dir):
    """Print the band table and the Hausdorff summary and write boundary_bands.json / .csv (one row per
    distance band), patch_boundary.csv (one row per patch) and patch_boundary.json (the summary)."""
    from . import metrics as MT

    doc = MT.boundary_report_summary(rows)
    doc["tolerance"] = tolerance
    print('    boundary report: pixels, coverage and risk by distance d to the label contour')
    print('    ' + ' '.join(f'{c:>14}' for c in ("band", "pixel_share", "coverage", "risk", "rejected_share",
                                                  "error_share")))
    for r in bands:
        name = ("no contour" if r["r_lo"] != r["r_lo"] else
                f'd > {r["r_lo"]:g}' if r["r_hi"] == float("inf") else f'{r["r_lo"]:g} < d <= {r["r_hi"]:g}')
        print('    ' + f'{name:>14} ' + ' '.join(f'{r[c]:14.6f}' for c in ("pixel_share", "coverage", "risk",
                                                                               "rejected_share", "error_share")))
    print(f'    Hausdorff distance over {doc["patches"]} patches: mean {doc["mean_hausdorff"]:.6f} median '
          f'{doc["median_hausdorff"]:.6f} ({doc["infinite_hausdorff"]} infinite, {doc["zero_hausdorff"]} zero)')
    os.makedirs(save_dir, exist_ok=True)
    _write_json(save_dir, "boundary_bands.json", {"radii": list(radii), "bands": bands})
    _write_csv(save_dir, "boundary_bands.csv", MT.BAND_COLUMNS, ([r[c] for c in MT.BAND_COLUMNS] for r in bands))
    cols = MT.boundary_report_columns(rows)
    _write_csv(save_dir, "patch_boundary.csv", cols, ([r[c] for c in cols] for r in rows))
    _write_json(save_dir, "patch_boundary.json", doc)
    return dict(doc, bands=bands, rows=rows)


def report_patches(rows, save_dir):
    """Print the per-patch summary and write patch_performance.csv (one row per patch, floats by repr)
    and patch_performance.json (the summary)."""
    from . import metrics as MT

    doc = MT.patch_report_summary(rows)
    print(f'    per-patch report: {doc["patches"]} patches, {doc["nan_auc"]} without an AUC (one class only), '
          f'AUC mean {doc["mean_auc"]:.6f} median {doc["median_auc"]:.6f}')
    os.makedirs(save_dir, exist_ok=True)
    cols = MT.patch_report_columns(rows)
    _write_csv(save_dir, "patch_performance.csv", cols, ([r[c] for c in cols] for r in rows))
    _write_json(save_dir, "patch_performance.json", doc)
    return dict(doc, rows=rows)


CSV_COLUMNS = ("s_cut_off", "coverage", "rejection_ratio", "selected", "total", "risk", "Acc", "mIoU")


def report_sweep(curve, target_coverage, save_dir):
    """Print the risk-coverage table and write risk_coverage.json / risk_coverage.csv."""
    from . import metrics as MT

    doc = {"curve": curve}
    print('    risk-coverage sweep of the selection cut-off:')
    print('    ' + ' '.join(f'{c:>12}' for c in ("s_cut_off", "coverage", "risk", "mIoU")))
    for r in curve:
        print('    ' + ' '.join(f'{r[c]:12.6f}' for c in ("s_cut_off", "coverage", "risk", "mIoU")))
    if target_coverage is not None:
        cut = MT.cut_off_for_coverage(curve, target_coverage)
        doc["target_coverage"] = target_coverage
        doc["calibrated_s_cut_off"] = cut
        doc["calibrated"] = None if cut is None else next(r for r in curve if r["s_cut_off"] == cut)
        if cut is None:
            doc["calibration_note"] = (f"coverage {target_coverage} is unreachable: the smallest cut-off "
                                       f"{curve[0]['s_cut_off']} covers {curve[0]['coverage']}")
            print(f'    target coverage {target_coverage}: unreachable (smallest cut-off '
                  f'{curve[0]["s_cut_off"]} covers {curve[0]["coverage"]:.6f})')
        else:
            r = doc["calibrated"]
            print(f'    target coverage {target_coverage}: s_cut_off {cut} (coverage {r["coverage"]:.6f}, '
                  f'risk {r["risk"]:.6f}, mIoU {r["mIoU"]:.6f})')
    os.makedirs(save_dir, exist_ok=True)
    _write_json(save_dir, "risk_coverage.json", doc)
    _write_csv(save_dir, "risk_coverage.csv", CSV_COLUMNS + ("cm00", "cm01", "cm10", "cm11"),
               ([r[c] for c in CSV_COLUMNS] + [int(v) for row in r["confusion_matrix"] for v in row] for r in curve))
    return doc


def main(argv=None):
    args = parse_arguments(sys.argv[1:] if argv is None else argv)
    print('')
    hidden = ()  # without a sweep / a patch report / the split path the printed line is what it was before these flags
    if sweep_cut_offs(args) is None:
        hidden += ('s_cut_off_sweep', 's_cut_off_steps', 'target_coverage')
    if not args.patch_report:
        hidden += ('patch_report',)
    if args.fp32_path == 'exact':
        hidden += ('fp32_path',)
    shown = argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in hidden})
    print('args={}\n'.format(shown))
    evaluate(args)
    return 0


if __name__ == '__main__':
    sys.exit(main())
