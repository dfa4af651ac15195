"""selunet_reduce_rows over its split plan, and the multi-tensor Adam at the size of the model's table.

selunet_reduce_rows (every loss goes through it with cols = 1 or 2, the BN reductions with up to 3 x 512) had one
kernel test, 3001 x 70: here the plan splits = min(128, cdiv(rows, 16)) runs from one split to the cap, with its
empty trailing splits (rows = 2049: chunk 17, splits 121..127 start past the end), one to four column blocks, and
the fp32 output. selunet_adam_step had one test of three tensors comparing parameters: here 68 tensors (the model's
count) whose sizes straddle the 4096-element chunk, both moments, and optim.py's table cache and per-step grouping.
"""
import numpy as np
import pytest
import torch

import selectivenet_for_semantic_segmentation_binary_amd as S
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from tests.test_gpu_kernels import gen, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
RED_SPLITS = 128  # csrc/pointwise.hip:243 constexpr int RED_SPLITS
ROWS = [1, 15, 16, 17, 127, 128, 129, 2047, 2048, 2049, 8192]
COLS = [1, 2, 63, 64, 65, 195]


def cdiv(a, b):
    return -(-a // b)


@pytest.mark.parametrize("rows", ROWS)
def test_reduce_rows_split_plan(rows):
    """Against the numpy fp64 column sums within test_reduce_rows_deterministic's 1e-12; out32 == float32(out),
    also where only out32 is given; two runs bit-identical."""
    splits = min(RED_SPLITS, cdiv(rows, 16))
    chunk = cdiv(rows, splits)
    assert (rows == 2049) == (splits * chunk - rows >= chunk)  # whole splits past the end, at 2049 only
    worst = 0.0
    for cols in COLS:
        slab = gen(rows, cols, seed=27 + cols).to(DEV)
        want = slab.cpu().numpy().astype(np.float64).sum(0)
        ws = torch.full((K.query("selunet_reduce_ws_bytes", cols) // 8,), float("nan"), dtype=torch.float64, device=DEV)
        runs = []
        for _ in range(2):
            o = torch.full((cols,), float("nan"), dtype=torch.float64, device=DEV)
            o32 = torch.full((cols,), float("nan"), device=DEV)
            only32 = torch.full((cols,), float("nan"), device=DEV)
            K.call("selunet_reduce_rows", K.ptr(slab), rows, cols, K.ptr(ws), K.ptr(o), K.ptr(o32), K.stream_ptr())
            K.call("selunet_reduce_rows", K.ptr(slab), rows, cols, K.ptr(ws), None, K.ptr(only32), K.stream_ptr())
            torch.cuda.synchronize()
            runs.append((o.cpu(), o32.cpu(), only32.cpu()))
        (o, o32, only32), second = runs
        assert all(torch.equal(a, b) for a, b in zip(runs[0], second))
        assert torch.equal(o32, o.float()) and torch.equal(only32, o32)
        err = rel(o, torch.tensor(want))
        worst = max(worst, err)
        assert err < 1e-12, (cols, err)
    print(f"coverage: reduce_rows rows={rows}: {worst:.2e} (bound 1.0e-12)")


# ------------------------------------------------------------------ Adam
NUMELS = [1, 3, 64, 4095, 4096, 4097, 2 * 4096, 36864]


def adam_pair(numels, groups=None, **kw):
    """Device parameters under S.Adam and CPU copies under torch.optim.Adam; groups: list of (slice, lr)."""
    g = torch.Generator().manual_seed(3)
    base = [torch.randn(n, generator=g) for n in numels]
    dev = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    ref = [b.clone().requires_grad_() for b in base]
    if groups is None:
        return dev, ref, S.Adam(dev, **kw), torch.optim.Adam(ref, **kw)
    return (dev, ref, S.Adam([dict(params=dev[sl], lr=lr) for sl, lr in groups], **kw),
            torch.optim.Adam([dict(params=ref[sl], lr=lr) for sl, lr in groups], **kw))


def set_grads(dev, ref, step, skip=(), keep=None):
    """New gradient tensors every step (the previous ones stay alive in `keep`, so the new ones have new addresses
    and the table cache must rebuild); skip: parameters whose grad is None this step."""
    g = torch.Generator().manual_seed(100 + step)
    for i, (p, r) in enumerate(zip(dev, ref)):
        gr = torch.randn(p.shape, generator=g) * (step + 1)
        if i in skip:
            p.grad = r.grad = None
            continue
        if keep is not None and p.grad is not None:
            keep.append(p.grad)
        p.grad = gr.to(DEV)
        r.grad = gr.clone()


def check_adam(tag, dev, ref, opt, ropt):
    worst = {}
    for p, r in zip(dev, ref):
        pairs = [("param", p.detach().cpu(), r.detach())]
        if p in opt.state:
            assert float(opt.state[p]["step"]) == float(ropt.state[r]["step"])
            pairs += [(k, opt.state[p][k].cpu(), ropt.state[r][k]) for k in ("exp_avg", "exp_avg_sq")]
        else:
            assert r not in ropt.state or len(ropt.state[r]) == 0
        for k, a, b in pairs:
            # the margin torch.allclose(rtol = atol = 1e-6) leaves, as a fraction of its bound
            worst[k] = max(worst.get(k, 0.0), float(((a - b).abs() / (1e-6 + 1e-6 * b.abs())).max()))
            assert torch.allclose(a, b, rtol=1e-6, atol=1e-6), (tag, k, p.numel(), worst[k])
    for k, v in worst.items():
        print(f"coverage: adam {tag} {k}: {v:.2e} of the allclose bound (bound 1.0e+00)")


def test_adam_68_tensors_both_moments():
    """One group of 68 tensors (the model's count), sizes on both sides of the 4096-element chunk; 3 steps with
    weight_decay 0.01: parameter, exp_avg and exp_avg_sq against torch.optim.Adam on the CPU
    (test_adam_matches_reference_algorithm's rtol = atol = 1e-6)."""
    numels = (NUMELS * 9)[:68]
    assert len(numels) == 68 and set(NUMELS) <= set(numels)
    dev, ref, opt, ropt = adam_pair(numels, lr=1e-2, weight_decay=0.01)
    for step in range(3):
        set_grads(dev, ref, step)
        opt.step()
        ropt.step()
    check_adam("68 tensors", dev, ref, opt, ropt)


def test_adam_grad_none_splits_the_launch_and_tables_rebuild():
    """A parameter in the middle has no gradient on step 2: its step count falls behind, so optim.py's by_step
    splits the group into two launches from step 3 on (two bias corrections); every step brings new gradient
    tensors at new addresses, so the cached device table must be rebuilt."""
    numels = NUMELS + NUMELS[::-1]
    mid = 7
    dev, ref, opt, ropt = adam_pair(numels, lr=1e-2, weight_decay=0.01)
    keep, ptrs = [], []
    for step in range(4):
        set_grads(dev, ref, step, skip=(mid,) if step == 1 else (), keep=keep)
        ptrs.append(dev[0].grad.data_ptr())
        opt.step()
        ropt.step()
    assert len(set(ptrs)) == len(ptrs)  # the gradients did move
    assert float(opt.state[dev[mid]]["step"]) == 3.0 and float(opt.state[dev[0]]["step"]) == 4.0
    check_adam("grad None / new grads", dev, ref, opt, ropt)


def test_adam_two_groups_and_preset_step():
    """Two param groups with different lr (one launch each), and states whose step is preset to 9999 (bias
    corrections 1 - beta^10000) with non-zero moments."""
    numels = NUMELS * 2
    dev, ref, opt, ropt = adam_pair(numels, groups=[(slice(0, 8), 1e-2), (slice(8, 16), 3e-4)], weight_decay=0.01)
    g = torch.Generator().manual_seed(5)
    for i in (2, 5, 12):
        m, v = torch.randn(numels[i], generator=g) * 0.1, torch.rand(numels[i], generator=g) * 0.01
        opt.state[dev[i]] = dict(step=torch.tensor(9999.0), exp_avg=m.to(DEV), exp_avg_sq=v.to(DEV))
        ropt.state[ref[i]] = dict(step=torch.tensor(9999.0), exp_avg=m.clone(), exp_avg_sq=v.clone())
    for step in range(3):
        set_grads(dev, ref, step)
        opt.step()
        ropt.step()
    assert float(opt.state[dev[5]]["step"]) == 10002.0
    check_adam("two groups / step 9999", dev, ref, opt, ropt)
