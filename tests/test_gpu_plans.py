"""Launch-plan replay (engine.py): a replayed training step must compute what the recorded
(Python-sequenced) step computes. Plans on vs off over several Adam steps; per-call outputs are
not aliased across steps; a forward whose graph is dropped without backward frees its plan.

Tolerance: the forward (convs, deterministic two-level BN reductions, heads) is bit-reproducible,
so with frozen weights (lr=0) a replayed forward must equal the recorded one bit for bit. The
weight-gradient kernels accumulate with fp32 atomics (summation order varies run to run), so
over real Adam steps runs agree to fp32 rounding, not bit for bit: step-0 head outputs 1e-4
relative (nothing has been updated yet); later steps' outputs 1e-2 relative to the tensor max and
parameters within 5e-3 absolute (Adam normalises the update, so an element whose gradient is
rounding noise moves by up to +-lr per step either way — the same bound the reference-parity
tests use for later steps). Losses: steps 0-1 within 1e-6 relative, step 2 within 1e-5, with the BN
statistics unshifted on both paths.
"""
import gc

import numpy as np
import pytest
import torch

import selectivenet_for_semantic_segmentation_binary_amd as S
from oracle import unet_b_cpu as O
from selectivenet_for_semantic_segmentation_binary_amd.synthetic import make_batch
from tests import _golden as G
from tests.test_gpu_model import build

pytestmark = pytest.mark.gpu


def _run(plans, steps=3, n=2, size=64, seed=0, lr=1e-3, same_batch=False):
    net = build(True, seed)
    net._engine().plans_enabled = plans
    opt = S.Adam(net.parameters(), lr=lr)
    loss_A = S.BCEWithLogitsLoss()
    losses, outs = [], []
    for s in range(steps):
        x, lab = make_batch(n, size, seed=10 + (0 if same_batch else s))
        xt, lt = torch.tensor(x, device="cuda"), torch.tensor(lab, device="cuda")
        o, sel, aux = net(xt)
        loss = loss_A(aux, lt) + S.calc_selective_risk_image_b(o, sel, target=lt, lamb=2)[0]
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        outs.append(o)  # held across steps: must keep this step's values
    snap = [o.detach().cpu().numpy().copy() for o in outs]
    params = {k: p.detach().cpu().numpy() for k, p in net.named_parameters()}
    return np.array(losses), snap, params, net


def test_replayed_steps_match_recorded_steps(monkeypatch):
    # unshifted BN statistics (SELUNET_BN_SHIFT=0): with the default shift a replayed step centres its
    # sums on the previous step's mean while the first recorded one uses 0, so the two paths would
    # differ in statistics rounding by design (test_replay_with_bn_shift_matches_to_rounding covers it)
    monkeypatch.setenv("SELUNET_BN_SHIFT", "0")
    l_on, o_on, p_on, net = _run(True)
    l_off, o_off, p_off, _ = _run(False)
    eng = net._engine()
    assert sum(len(v) for v in eng._plans.values()) >= 1 and all(e.plan is not None for v in eng._plans.values()
                                                                   for e in v)
    assert np.allclose(l_on[:2], l_off[:2], rtol=1e-6, atol=0), (l_on, l_off)
    assert np.allclose(l_on[2:], l_off[2:], rtol=1e-5, atol=0), (l_on, l_off)
    assert np.abs(o_on[0] - o_off[0]).max() <= 1e-4 * max(1.0, np.abs(o_off[0]).max())
    for a, b in zip(o_on[1:], o_off[1:]):
        assert np.abs(a - b).max() <= 1e-2 * max(1.0, np.abs(b).max())
    # outputs of different steps differ (no aliasing of a plan-owned buffer)
    assert not np.array_equal(o_on[0], o_on[1])
    for k in p_on:
        assert np.abs(p_on[k] - p_off[k]).max() <= 5e-3, k


def test_replay_with_frozen_weights_is_bit_exact(monkeypatch):
    # lr=0: parameters never move, the batch repeats, so step 0 (recorded) and steps 1-2
    # (replayed) run the same forward on the same inputs and must agree bit for bit — with the BN
    # statistics unshifted (SELUNET_BN_SHIFT=0: the shifted sums of the default depend on the previous
    # step's mean, test_replay_with_bn_shift_matches_to_rounding)
    monkeypatch.setenv("SELUNET_BN_SHIFT", "0")
    l_on, o_on, _, net = _run(True, lr=0.0, same_batch=True)
    assert all(e.plan is not None for v in net._engine()._plans.values() for e in v)
    for o in o_on[1:]:
        assert np.array_equal(o, o_on[0])
    assert l_on[1] == l_on[0] and l_on[2] == l_on[0]


def test_replay_with_bn_shift_matches_to_rounding():
    """The default fp32 BN statistics (engine.Engine.bn_shift): the conv epilogue sums y - c with c =
    the previous step's batch mean. With frozen weights and a repeated batch, steps 1-2 (c = the mean
    step 0 found) must reproduce step 0 (c = 0) to the rounding of the statistics: outputs within
    1e-5 relative to the tensor max, loss within 1e-6 relative."""
    l_on, o_on, _, net = _run(True, lr=0.0, same_batch=True)
    assert net._engine().bn_shift
    for o in o_on[1:]:
        assert np.abs(o - o_on[0]).max() <= 1e-5 * max(1.0, np.abs(o_on[0]).max())
    assert np.allclose(l_on, l_on[0], rtol=1e-6, atol=0), l_on


def test_replay_with_stale_bn_center_matches_oracle():
    """The case the shifted statistics are built for: frozen weights (lr = 0, so no trajectory effect can hide
    behind rounding) and a new batch every step, so replayed step k centres its sums on the mean of batch k - 1.
    Every step's output against the CPU oracle's fp32 training forward of that batch on the same weights (the
    project's forward tolerance, 1e-4 of the tensor max); after step 4 every running_mean / running_var against
    the oracle's fp64 buffers, no further than max(3 x the oracle's own fp32 deviation from fp64, 1e-5) relative
    to the buffer's max (the yardstick of tests/_golden.check_grads_vs_truth); and against the same four steps
    with plans off (a zero center at every step) within the 1e-5 of test_replay_with_bn_shift_matches_to_rounding.
    Measured on the MI355X: outputs within 2.30e-6 (replayed) and 2.34e-6 (plans off) of the oracle's fp32 run,
    replayed within 1.66e-6 of plans off (0 at step 0), the worst running statistic at 0.018 of its bound
    (every bound is the 1e-5 floor: the oracle's own fp32 buffers deviate from fp64 by 6e-8 .. 2.9e-7)."""
    steps = 4
    _, o_on, _, net_on = _run(True, lr=0.0, same_batch=False, steps=steps)
    _, o_off, _, net_off = _run(False, lr=0.0, same_batch=False, steps=steps)
    eng = net_on._engine()
    assert eng.bn_shift and all(e.plan is not None for v in eng._plans.values() for e in v)
    state = {}
    for dt in (torch.float32, torch.float64):
        params, buffers = O.make_state(0, "RGB", True)
        params = {k: v.detach().to(dt) for k, v in params.items()}
        buffers = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in buffers.items()}  # carried over the steps
        outs = []
        with torch.no_grad():
            for s in range(steps):
                x, _ = make_batch(2, 64, seed=10 + s)
                outs.append(O.forward(params, buffers, torch.tensor(x, dtype=dt), True, training=True)[0].numpy())
        state[dt] = (outs, buffers)
    o32, b32 = state[torch.float32]
    o64, b64 = state[torch.float64]
    worst_out = worst_off = worst_pair = 0.0
    for s in range(steps):
        e_on, e_off = G.max_rel(o_on[s], o32[s]), G.max_rel(o_off[s], o32[s])
        pair = np.abs(o_on[s] - o_off[s]).max() / max(1.0, np.abs(o_off[s]).max())
        print(f"step {s}: output vs oracle fp32: replayed {e_on:.2e}, eager {e_off:.2e} (vs oracle fp64: "
              f"{G.max_rel(o_on[s], o64[s]):.2e}, {G.max_rel(o_off[s], o64[s]):.2e}); replayed vs eager {pair:.2e}")
        worst_out, worst_off, worst_pair = max(worst_out, e_on), max(worst_off, e_off), max(worst_pair, pair)
    worst_ratio = 0.0
    fails = []
    for net, tag in ((net_on, "replayed"), (net_off, "eager")):
        for k, v in net.named_buffers():
            if k.endswith("num_batches_tracked"):
                assert int(v) == steps, k
            if "running" not in k:
                continue
            bound = max(3.0 * G.max_rel(b32[k].numpy(), b64[k].numpy()), 1e-5)
            dev = G.max_rel(v.cpu().numpy(), b64[k].numpy())
            worst_ratio = max(worst_ratio, dev / bound)
            if dev > bound:
                fails.append(f"{tag} {k}: {dev:.2e} > {bound:.2e}")
    print(f"worst output deviation vs oracle fp32: replayed {worst_out:.2e}, eager {worst_off:.2e}; replayed vs "
          f"eager {worst_pair:.2e}; worst running-statistic deviation / bound {worst_ratio:.3f}")
    assert worst_out < 1e-4 and worst_off < 1e-4
    assert not fails, "\n".join(fails)
    assert worst_pair <= 1e-5
    assert not np.array_equal(o_on[0], o_on[1])  # (the batches do differ)


def test_dropped_graph_releases_plan_and_eval_forward_replays():
    net = build(True, 0)
    eng = net._engine()
    x, lab = make_batch(2, 32, seed=3)
    xt = torch.tensor(x, device="cuda")
    o, s, a = net(xt)  # training forward, graph kept...
    entries = [e for v in eng._plans.values() for e in v]
    assert len(entries) == 1 and entries[0].busy
    del o, s, a  # ...then dropped without backward
    gc.collect()
    assert not entries[0].busy
    net.eval()
    with torch.no_grad():
        r1 = net(xt)[0].clone()
        r2 = net(xt)[0]  # replay of the eval plan
    assert torch.equal(r1, r2)
