"""Host side of the fp32 eval conv path option (no GPU): the two CLIs' flags, the printed args line, the module
keyword / attribute and the path report."""
import argparse

import pytest
import torch

import selectivenet_for_semantic_segmentation_binary_amd as S
from selectivenet_for_semantic_segmentation_binary_amd import eval as EV
from selectivenet_for_semantic_segmentation_binary_amd import train as TR
from selectivenet_for_semantic_segmentation_binary_amd.engine import EVAL_PATHS, check_eval_path, fp32_eval_conv_path


def test_defaults():
    assert EV.parse_arguments([]).fp32_path == "exact"
    assert TR.parse_arguments([]).valid_fp32_path == "exact"
    assert EV.parse_arguments(["--fp32_path", "split"]).fp32_path == "split"
    assert TR.parse_arguments(["--valid_fp32_path", "split"]).valid_fp32_path == "split"
    assert EVAL_PATHS == ("exact", "split")
    for net in (S.UNet_B("RGB", selective=True), S.UNet("RGB", 2, selective=True)):
        assert net.fp32_eval_path == "exact"
    assert S.UNet_B("RGB", True, torch.float32, "split").fp32_eval_path == "split"  # the documented positional order
    assert S.UNet("RGB", 2, True, fp32_eval_path="split").fp32_eval_path == "split"


@pytest.mark.parametrize("cli,flag", [(EV, "--fp32_path"), (TR, "--valid_fp32_path")])
def test_cli_refusals(cli, flag, capsys):
    with pytest.raises(SystemExit):
        cli.parse_arguments([flag, "split", "--compute_dtype", "bf16"])
    assert "bf16" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse_arguments([flag, "fast"])
    capsys.readouterr()
    assert cli.parse_arguments([flag, "exact", "--compute_dtype", "bf16"]).compute_dtype == "bf16"


def printed_args_line(module, argv, monkeypatch, capsys, entry):
    """The `args=` line main() prints, with the work behind it stubbed out."""
    monkeypatch.setattr(module, entry, lambda *a, **k: None)
    module.main(argv)
    return next(ln for ln in capsys.readouterr().out.split("\n") if ln.startswith("args="))


def test_eval_printed_line_unchanged_when_exact(monkeypatch, capsys):
    argv = ["--selective", "1", "--batch_size", "4"]
    line = printed_args_line(EV, argv, monkeypatch, capsys, "evaluate")
    assert "fp32_path" not in line
    # ... and is the line of a parser without the flag: the namespace minus the hidden entries, in argparse's order
    args = EV.parse_arguments(argv)
    hidden = ("s_cut_off_sweep", "s_cut_off_steps", "target_coverage", "patch_report", "fp32_path")
    want = argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in hidden})
    assert line == "args={}".format(want)
    assert printed_args_line(EV, argv + ["--fp32_path", "exact"], monkeypatch, capsys, "evaluate") == line
    on = printed_args_line(EV, argv + ["--fp32_path", "split"], monkeypatch, capsys, "evaluate")
    assert "fp32_path='split'" in on and on.replace(", fp32_path='split'", "") == line


def test_train_printed_line_unchanged_when_exact(monkeypatch, capsys):
    argv = ["--model_arch", "UNet_B", "--loss", "BCElogit"]
    line = printed_args_line(TR, argv, monkeypatch, capsys, "train")
    assert "valid_fp32_path" not in line
    args = TR.parse_arguments(argv)
    want = argparse.Namespace(**{k: v for k, v in vars(args).items() if k != "valid_fp32_path"})
    assert line == "args={}".format(want)
    on = printed_args_line(TR, argv + ["--valid_fp32_path", "split"], monkeypatch, capsys, "train")
    assert on.replace(", valid_fp32_path='split'", "") == line and on != line


def test_unknown_path_is_a_value_error():
    for make in (lambda: S.UNet_B("RGB", selective=True, fp32_eval_path="fast"),
                 lambda: S.UNet("RGB", 2, selective=False, fp32_eval_path=None),
                 lambda: check_eval_path("Split"), lambda: fp32_eval_conv_path("winograd")):
        with pytest.raises(ValueError):
            make()
    net = S.UNet_B("RGB", selective=False)
    net.fp32_eval_path = "split"
    with pytest.raises(ValueError):
        net.fp32_eval_path = ""
    assert net.fp32_eval_path == "split"
    assert "fp32_eval_path" not in "".join(net.state_dict().keys())  # not state: checkpoints are unchanged


def test_path_report(monkeypatch):
    monkeypatch.delenv("SELUNET_X2", raising=False)
    monkeypatch.delenv("SELUNET_WINO", raising=False)
    assert fp32_eval_conv_path() == "exact-fp32 (Winograd)"
    assert fp32_eval_conv_path("split") == "split-fp16"
    assert fp32_eval_conv_path("split", torch.bfloat16) == "bf16"
    monkeypatch.setenv("SELUNET_X2", "0")
    assert fp32_eval_conv_path("split") == "exact-fp32 (Winograd)"
    monkeypatch.setenv("SELUNET_WINO", "0")
    assert fp32_eval_conv_path("split") == "exact-fp32 (direct)"
