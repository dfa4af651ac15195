"""CPU emulation of the split-fp16 operand format under loose range words.

The split-fp16 kernels scale every operand by a power of two taken from a device range word (x2_scale: the largest
2^e with amax * 2^e < 2^14; 2^14 for amax = 0), split it as v * 2^e = h + l with h = fp16(v * 2^e), l = fp16(v * 2^e
- h) (x2_split), and sum h_a h_b + h_a l_b + l_a h_b. In training the word of a BN+ReLU source is the Samuelson
bound |gamma| sqrt(M) + |beta|, 2^9..2^10 above the real maximum at 128 x 256^2: operands sit that much lower in the
fp16 range, and their low parts go subnormal earlier.

This emulates the operand format alone (numpy float16 splits, the three products summed in fp64, K = 2304) and
bounds its error against the fp64 product of the unsplit fp32 operands. It is the reference the GPU tests' bound
rests on when they pass range words 2^10 and 2^12 above the true maximum at an unchanged tolerance of 2e-6
(tests/test_gpu_x2.py::SLACKS) — not the kernel under test. Measured here: 7.8e-8 of the output maximum at slack
1, 7.6e-8 at 2^10, 8.2e-8 at 2^12, 9.6e-6 at 2^20.
"""
import numpy as np
import pytest

K_DIM, ROWS, COLS = 2304, 64, 64


def x2_scale(amax):
    """The power of two the kernels scale an operand with: amax * 2^e < 2^14 (2^14 for an all-zero operand)."""
    if amax == 0:
        return 2.0 ** 14
    _, e = np.frexp(np.float32(amax))  # amax = m * 2^e, 0.5 <= m < 1
    return 2.0 ** (14 - int(e))


def x2_split(v, scale):
    s = (v.astype(np.float32) * np.float32(scale)).astype(np.float32)
    h = s.astype(np.float16)
    lo = (s - h.astype(np.float32)).astype(np.float16)
    return h.astype(np.float64), lo.astype(np.float64)


def operand_error(slack, seed=0):
    """Relative (to the output maximum) error of the split product of an activation-like A [ROWS][K] (half of it
    zero, as after a ReLU) and a weight-like B [COLS][K] whose rows carry their own exact scales."""
    rng = np.random.default_rng(seed)
    a = np.maximum(rng.standard_normal((ROWS, K_DIM)), 0).astype(np.float32)
    b = (rng.standard_normal((COLS, K_DIM)) * 0.05).astype(np.float32)
    sa = x2_scale(float(np.abs(a).max()) * slack)
    ah, al = x2_split(a, sa)
    sb = np.array([x2_scale(float(np.abs(r).max())) for r in b])
    bh, bl = x2_split(b, sb[:, None])
    got = (ah @ bh.T + ah @ bl.T + al @ bh.T) / sa / sb[None, :]
    ref = a.astype(np.float64) @ b.astype(np.float64).T
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def test_scale_keeps_operands_in_range():
    for amax in (1e-9, 0.3, 1.0, 2.0, 5.7, 16384.0, 3e7):
        s = x2_scale(amax)
        assert amax * s < 2.0 ** 14 <= amax * s * 2
    assert x2_scale(0.0) == 2.0 ** 14


@pytest.mark.parametrize("slack", [1.0, 2.0 ** 10, 2.0 ** 12])
def test_split_error_up_to_training_slack(slack):
    err = operand_error(slack)
    print(f"slack 2^{int(np.log2(slack))}: operand-only error {err:.2e}")
    assert err <= 2e-7


def test_split_error_shows_at_large_slack():
    """The emulation is sensitive: at slack 2^20 the low parts are lost and the error passes the GPU bound."""
    err = operand_error(2.0 ** 20)
    print(f"slack 2^20: operand-only error {err:.2e}")
    assert err > 2e-6


def test_zero_operand_is_exact():
    h, lo = x2_split(np.zeros((4, 32), np.float32), x2_scale(0.0))
    assert not h.any() and not lo.any()
